"""Helpers shared by the kernel-level GPU tests (test_00, test_05, test_06): the error metric, fp16 random inputs, the Python mirror of
csrc/common.h's dropout hash, and the product / investigation gating of the NT GEMM variants.  One definition, imported by all."""
import pytest
import torch

from vlp_amd import _lib as K

from tests.hard_inputs import attn_mask, attn_ref, rel      # noqa: F401   (library-free: shared with the CPU tests)

DEV = torch.device("cuda:0")
M32 = 0xFFFFFFFF


# ---- python mirror of csrc/common.h's dropout hash (uint32 arithmetic on int64 tensors) -----------------
def _mix32(x):
    x = x & M32
    x = x ^ (x >> 15); x = ((x & 0xFFFFFF) * 0xd3833f + (x >> 7)) & M32
    x = x ^ (x >> 13); x = ((x & 0xFFFFFF) * 0x7a6b35 + (x >> 9)) & M32
    x = x ^ (x >> 16)
    return x


def _mul64(a, b):
    return (a * b) & 0xFFFFFFFFFFFFFFFF


def drop_mult_ref(p, seed, stream, rows, cols, device=DEV):
    """[len(rows), len(cols)] multiplier tensor (0 or 1/(1-p)) for elements (row, col): one hash per column pair, the even column
    takes the low 16 bits, the odd one the high 16 bits, dropped when that half is below round(p * 65536)."""
    if p <= 0:
        return torch.ones(len(rows), len(cols), device=device)
    s = (_mul64(seed, 0x9E3779B97F4A7C15) + _mul64(stream, 0xD1B54A32D192ED03) + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = s & M32, ((s >> 32) & M32) | 1
    thresh = min(65535, max(1, int(p * 65536.0 + 0.5)))
    rows = torch.as_tensor(rows, dtype=torch.int64, device=device)
    cols = torch.as_tensor(cols, dtype=torch.int64, device=device)
    rk = (_mix32((rows & M32) ^ k0) + _mix32(((rows >> 32) & M32) + k1)) & M32
    h = _mix32((rk[:, None] + ((cols[None, :] >> 1) * 0x9E3779B9 & M32)) & M32)
    half = torch.where((cols[None, :] & 1) == 1, h >> 16, h & 0xFFFF)
    return torch.where(half < thresh, torch.zeros((), device=device), torch.full((), 1.0 / (1.0 - p), device=device))


def h16(*shape, scale=1.0, gen=None):
    return (torch.randn(*shape, device=DEV, generator=gen) * scale).half()


# Investigation variants (phased / k32 NT kernels, further wave-pipelined configurations, two-kernel and exchange-tile attention
# backward, stream-K grouped wgrad) live in -DVLP_LAB_BUILD libraries only (`python -m vlp_amd.build --lab`, VLP_HIP_LIB=vlp_amd/libvlp_hip_lab.so):
# against the product library their cases are not collected as work, they skip.
LAB = K.lab_build()
NT_PRODUCT = {0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 17, 19, 21, 27, 29, 65, 69, 73, 77, 256, 264}


def nt_variants(vs):
    return [v if (LAB or v in NT_PRODUCT) else pytest.param(v, marks=pytest.mark.skip(reason="investigation variant: needs a -DVLP_LAB_BUILD library")) for v in vs]

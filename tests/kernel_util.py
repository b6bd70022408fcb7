"""Helpers shared by the kernel-level GPU tests (test_00, test_05, test_06, test_32): the error metric, fp16 random inputs, the Python mirror of
csrc/common.h's dropout hash, the fp64 restatement of the fused Adam update, and the product / investigation gating of the NT GEMM variants.
One definition, imported by all."""
import pytest
import torch

from vlp_amd import _lib as K

from tests.dropout_ref import M32, _mix32, _mul64, drop_mult_ref as _drop_mult_ref      # noqa: F401
from tests.hard_inputs import attn_mask, attn_ref, rel      # noqa: F401   (library-free: shared with the CPU tests)

DEV = torch.device("cuda:0")


# ---- python mirror of csrc/common.h's dropout hash: tests/dropout_ref.py (library-free); here with this module's device as the default ----
def drop_mult_ref(p, seed, stream, rows, cols, device=DEV):
    return _drop_mult_ref(p, seed, stream, rows, cols, device)


def h16(*shape, scale=1.0, gen=None):
    return (torch.randn(*shape, device=DEV, generator=gen) * scale).half()


def _adam_ref(p, m, v, g, combined, step, b1=0.9, b2=0.999, eps=1e-8, decay=0.01):
    """fp64 restatement of include/vlp_hip.h's vlp_fused_adam (eps outside the sqrt)."""
    g = g.double() / combined
    m2 = b1 * m.double() + (1 - b1) * g
    v2 = b2 * v.double() + (1 - b2) * g * g
    p2 = p.double() - step * (m2 / (v2.sqrt() + eps) + decay * p.double())
    return p2, m2, v2


# Investigation variants (phased / k32 NT kernels, further wave-pipelined configurations, two-kernel and exchange-tile attention
# backward, stream-K grouped wgrad) live in -DVLP_LAB_BUILD libraries only (`python -m vlp_amd.build --lab`, VLP_HIP_LIB=vlp_amd/libvlp_hip_lab.so):
# against the product library their cases are not collected as work, they skip.
LAB = K.lab_build()
NT_PRODUCT = {0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 17, 19, 21, 27, 29, 65, 69, 73, 77, 256, 264}


def nt_variants(vs):
    return [v if (LAB or v in NT_PRODUCT) else pytest.param(v, marks=pytest.mark.skip(reason="investigation variant: needs a -DVLP_LAB_BUILD library")) for v in vs]

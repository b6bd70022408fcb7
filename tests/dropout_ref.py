"""Library-free Python mirror of the dropout of the fused step: the counter hash of vlp_amd/csrc/common.h and the table of dropout
sites of one training step.  Imports neither vlp_amd._lib nor a device, so the CPU tests (and the oracle's pinning against the
reference) use the same masks as the GPU tests.

THE CONTRACT (also DESIGN.md, "Dropout sites"): a step with seed s = engine.base_seed + engine.step_seed drops element (row, col) of
site X when the hash of (s, stream(X), row, col) falls below round(p * 65536); rows are LOGICAL (dense) rows, whatever the packing.

    site             tensor            row                          col      stream        p
    "vis"            [B*Nv, H]         b*Nv + n                     h        1001          hidden
    "vispe"          [B*Nv, H]         b*Nv + n                     h        1002          hidden
    "emb"            [B*L, H]          b*L + l                      h        1000          hidden
    ("attn", i)      [B, heads, L, L]  (b*heads + head)*L + query   key      16*i + 1      attention
    ("attn_out", i)  [B*L, H]          b*L + l                      h        16*i + 2      hidden
    ("ffn_out", i)   [B*L, H]          b*L + l                      h        16*i + 3      hidden

Forward and backward of the engine both follow it, and a resumed checkpoint replays it: the numbering cannot change."""
import torch

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


def drop_mult_ref(p, seed, stream, rows, cols, device):
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


# ---- the sites of one step ------------------------------------------------------------------------------
STREAM_VIS, STREAM_VISPE, STREAM_EMB = 1001, 1002, 1000


def stream_attn(i):
    return 16 * i + 1


def stream_attn_out(i):
    return 16 * i + 2


def stream_ffn_out(i):
    return 16 * i + 3


def site_table(B, L, Nv, H, heads, layers):
    """[(site, stream, rows, cols, shape, kind)] in the order the forward visits the sites; kind "hidden" | "attn" names the probability."""
    t = [("vis", STREAM_VIS, B * Nv, H, (B * Nv, H), "hidden"),
         ("vispe", STREAM_VISPE, B * Nv, H, (B * Nv, H), "hidden"),
         ("emb", STREAM_EMB, B * L, H, (B * L, H), "hidden")]
    for i in range(layers):
        t.append((("attn", i), stream_attn(i), B * heads * L, L, (B, heads, L, L), "attn"))
        t.append((("attn_out", i), stream_attn_out(i), B * L, H, (B * L, H), "hidden"))
        t.append((("ffn_out", i), stream_ffn_out(i), B * L, H, (B * L, H), "hidden"))
    return t


def site_order(layers):
    """The sites in the order one forward applies them (= the order the reference calls nn.Dropout)."""
    return [s[0] for s in site_table(1, 1, 1, 2, 1, layers)]


def step_masks(seed, p_hidden, p_attn, B, L, Nv, H, heads, layers, device="cpu"):
    """{site: fp32 multiplier tensor (0 or 1/(1-p))} of every dropout site of the step with this seed (see the table above)."""
    out = {}
    for site, stream, nr, nc, shape, kind in site_table(B, L, Nv, H, heads, layers):
        p = p_attn if kind == "attn" else p_hidden
        out[site] = drop_mult_ref(p, seed, stream, range(nr), range(nc), device).view(shape)
    return out


# ---- the bounds of the dropout-on step test (tests/test_15_dropout_step_gpu.py), shared with the CPU test that shows they discriminate ----
def grad_norm_bound(ref_norm, gscale):
    """| ||g|| - ||ref|| | of one parameter; gscale = the largest gradient norm of the step (tests/test_10_model_gpu.py, dropout 0)."""
    return 2e-2 * ref_norm + 2e-3 * gscale


def grad_tensor_bound(ref_norm, numel, gscale, yard_err=0.0):
    """|| g - ref || over the WHOLE tensor.  tests/test_10_model_gpu.py bounds a strided sample of n <= 4096 entries by 3e-2 ||sample|| +
    2e-3 gscale sqrt(n) / 64; the whole tensor keeps the relative term and the absolute term of a full 4096-entry sample (it does not grow
    with the tensor, so for a large tensor this is the tighter reading).  yard_err = || g_fp16_oracle - ref ||, the error of the
    reference's own fp16 arithmetic on the same tensor: 1.5 x that where it is larger, the factor the fixture tests use."""
    return max(3e-2 * ref_norm + 2e-3 * gscale * min(numel, 4096) ** 0.5 / 64.0, 1.5 * yard_err)

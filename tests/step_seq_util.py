"""Helpers of the step-sequence tests (tests/test_35_step_sequence_gpu.py): exact tensor comparison with a readable verdict, and the
derived bound of an accumulated fp16 gradient.  Only torch is imported; the CPU tests of this file run without a GPU."""
import torch

_BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def bit_diff(a, b):
    """Number of elements of `a` and `b` whose BITS differ (NaN == NaN of the same payload, +0 != -0: an overflow step must compare
    equal to itself, which torch.equal would deny); -1 for a shape / dtype mismatch."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return -1
    if a.dtype in _BITS:
        a, b = a.contiguous().view(_BITS[a.dtype]), b.contiguous().view(_BITS[b.dtype])
    return int((a != b).sum())


def first_difference(got, want):
    """got / want: ordered {name: tensor | python value | None}.  None if everything is equal, else a sentence naming the first entry that
    differs and how many of its elements do."""
    if list(got.keys()) != list(want.keys()):
        return "the two runs produced different outputs: %s against %s" % (sorted(got.keys()), sorted(want.keys()))
    for name, g in got.items():
        w = want[name]
        if torch.is_tensor(g) and torch.is_tensor(w):
            n = bit_diff(g, w)
            if n < 0:
                return "%s: %s %s against %s %s" % (name, tuple(g.shape), g.dtype, tuple(w.shape), w.dtype)
            if n:
                return "%s: %d of %d elements differ" % (name, n, g.numel())
        elif torch.is_tensor(g) or torch.is_tensor(w) or g != w:
            return "%s: %r against %r" % (name, g, w)
    return None


def fp16_ulp(x):
    """Spacing of the fp16 grid at |x| (x: any float tensor; result fp32): 2^(floor(log2 |x|) - 10), and 2^-24 -- the subnormal
    spacing -- below 2^-14."""
    x = x.detach().float().abs()
    _, e = torch.frexp(x)                     # |x| = m * 2^e, m in [0.5, 1)  ->  floor(log2 |x|) = e - 1  (frexp(0) = (0, 0): zero is handled apart)
    ulp = torch.ldexp(torch.ones_like(x), e - 11)
    return torch.where(x == 0, torch.full_like(x, 2.0 ** -24), torch.clamp(ulp, min=2.0 ** -24))


def accumulation_excess(acc, g1, g2, rounded):
    """An fp16 gradient tensor accumulated over two backward passes against the fp32 sum of the two single-step gradients.

    Every accumulating launch of the library computes `dst = rn16(float(dst) + e)` with e summed in fp32 (gemm_tn.hip, the partial-row
    reduce of layernorm.hip, copy2d and the table kernels of elementwise.hip): one fp32 add and one fp16 rounding, each wrong by at most
    half an fp16 ulp of the value it produced.  With one such launch per backward, acc = rn16(g1 + e2) and g2 = rn16(e2), so
    |acc - (g1 + g2)| <= ulp(acc) / 2 + ulp(g2) / 2  (<= 1 ulp at max(|acc|, |g2|)): rounded = (acc, g2).
    A tensor written by r launches per backward sees r roundings on either side, the earlier ones at the magnitude of the
    INTERMEDIATE value (which exceeds the final one where the launches' contributions cancel): `rounded` lists every rounded value,
    2 r tensors, and the bound is the sum of their half ulps.  (The fp32 add itself rounds to 2^-24 of the sum, at most 2^-13 of an
    fp16 ulp of the result: the factor 1 + 2^-13.)

    Returns (largest error / allowed, number of elements above the bound)."""
    a, x, y = acc.detach().double(), g1.detach().double(), g2.detach().double()
    err = (a - (x + y)).abs()
    allowed = sum(0.5 * fp16_ulp(t) for t in rounded).double() * (1.0 + 2.0 ** -13)
    ratio = err / allowed
    return (float(ratio.max()) if ratio.numel() else 0.0), int((err > allowed).sum())

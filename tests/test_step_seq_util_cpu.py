"""CPU: the comparison helpers of the step-sequence tests (tests/step_seq_util.py)."""
import torch

from tests.step_seq_util import accumulation_excess, bit_diff, first_difference, fp16_ulp


def test_fp16_ulp_is_the_grid_spacing():
    x = torch.tensor([1.0, 1.5, 1.9995, 2.0, 0.75, 2.0 ** -14, 2.0 ** -15, 0.0, 65504.0, -3.0])
    want = torch.tensor([2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 32.0, 2.0 ** -9])
    assert torch.equal(fp16_ulp(x), want)
    h = torch.tensor([1.0, 0.37, 1000.0, 6e-6], dtype=torch.float16)
    above = (h.view(torch.int16) + 1).view(torch.float16)           # the next fp16 value (positive inputs, none at the top of a binade)
    assert torch.equal(above.float() - h.float(), fp16_ulp(h))


def test_bit_diff_counts_bits_not_values():
    nan = torch.tensor([float("nan"), 1.0, 0.0], dtype=torch.float16)
    assert bit_diff(nan, nan.clone()) == 0 and not torch.equal(nan, nan.clone())
    assert bit_diff(torch.tensor([0.0]), torch.tensor([-0.0])) == 1
    assert bit_diff(torch.zeros(3), torch.zeros(4)) == -1 and bit_diff(torch.zeros(3), torch.zeros(3).half()) == -1
    assert bit_diff(torch.tensor([1, 2, 3]), torch.tensor([1, 5, 3])) == 1


def test_first_difference_names_the_tensor_and_the_count():
    a = {"loss": torch.ones(1), "grad w": torch.zeros(4, 4), "rows": 7}
    b = {"loss": torch.ones(1), "grad w": torch.zeros(4, 4), "rows": 7}
    assert first_difference(a, b) is None
    b["grad w"][1, 2:] = 1.0
    assert first_difference(a, b) == "grad w: 2 of 16 elements differ"
    b["grad w"].zero_()
    b["rows"] = None
    assert first_difference(a, b) == "rows: 7 against None"


def test_accumulation_bound_holds_for_the_kernels_arithmetic_and_bites_beyond_it():
    g = torch.Generator().manual_seed(0)
    e1, e2 = torch.randn(1 << 16, generator=g), torch.randn(1 << 16, generator=g) * 0.3
    e2[:4096] = -e1[:4096] * (1 + 1e-3)                       # cancellation: a small sum of large terms
    g1, g2 = e1.half(), e2.half()
    acc = (g1.float() + e2).half()                             # dst = rn16(float(dst) + e): one accumulating launch
    ratio, bad = accumulation_excess(acc, g1, g2, (acc, g2))
    assert bad == 0 and 0.4 < ratio <= 1.0
    off = (acc.view(torch.int16) + 2).view(torch.float16)      # two grid steps away
    assert accumulation_excess(off, g1, g2, (acc, g2))[1] > 50000    # (not all: where |g2| >> |acc| two steps of acc's grid are within ulp(g2) / 2)
    # two launches per backward (a, then b): the first rounding happens at the intermediate value
    a2, b2 = torch.randn(1 << 16, generator=g) * 4, torch.randn(1 << 16, generator=g)
    b2[:4096] = -a2[:4096]
    t = (g1.float() + a2).half()
    acc2 = (t.float() + b2).half()
    u = a2.half()
    s2 = (u.float() + b2).half()
    assert accumulation_excess(acc2, g1, s2, (t, acc2, u, s2))[1] == 0
    assert accumulation_excess(acc2, g1, s2, (acc2, s2))[1] > 0           # the one-launch bound is not valid for it

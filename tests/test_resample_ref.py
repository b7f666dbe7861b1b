"""tests/resample_ref.py proved before it judges a kernel (no GPU): against
scipy.signal.resample_poly on every case the GPU test uses, an f32 emulation of the
kernel's FMA chain that must stay under the bound, and wrong restatements that must
exceed it."""
import numpy as np
import pytest
from scipy.signal import resample_poly

from tests import resample_ref as R


CASES, case = R.CASES, R.case


@pytest.mark.parametrize("up,down,n", CASES)
def test_agrees_with_scipy(up, down, n):
    """scipy filters f32 input in f32 with the same taps rounded to f32: its own error is
    of the size of the bound, so the two are held to twice the bound."""
    x, y, bound = case(up, down, n)
    want = resample_poly(x, up, down)
    assert want.dtype == np.float32 and want.shape == y.shape == (R.out_len(n, up, down),)
    assert R.worst(want, y, bound, sides=2) <= 1


@pytest.mark.parametrize("up,down", R.RATIOS)
def test_impulses_agree_with_scipy(up, down):
    x, y, bound = case(up, down, 1000, impulse=True)
    assert R.worst(resample_poly(x, up, down), y, bound, sides=2) <= 1
    # the response of sample 0 is the taps at t0 = (m + rem) down, one rounding each
    P, h = R.plan(up, down), R.taps(up, down)
    t0 = (np.arange(len(y)) + P["rem"]) * down - P["pre"]
    m = np.nonzero((t0 >= 0) & (t0 < len(h)) & (t0 < (1000 - 1) * up - P["pre"] - len(h)))[0]
    assert m.size > 0 and np.array_equal(y[m], h[t0[m]])


def emulate(x, up, down):
    """The kernel's arithmetic: f32 taps, one f32 FMA per tap in ascending k (an f64
    product of two f32 values is exact; the f64 sum rounded to f32 can differ from a true
    FMA by double rounding, 2^-53 relative: far inside the bound)."""
    P = R.plan(up, down)
    hp = np.concatenate([np.zeros(P["pre"]), R.taps(up, down)]).astype(np.float32).astype(np.float64)
    n_in, n_out = len(x), R.out_len(len(x), up, down)
    x64 = np.asarray(x, np.float64)
    t0 = (np.arange(n_out, dtype=np.int64) + P["rem"]) * down
    p, q = t0 % up, t0 // up
    acc = np.zeros(n_out, np.float32)
    for j in range(P["J"]):
        k, i = p + j * up, q - j
        live = (k < len(hp)) & (i >= 0) & (i < n_in)
        term = np.where(live, hp[np.minimum(k, len(hp) - 1)] * x64[np.clip(i, 0, n_in - 1)], 0.0)
        acc = (term + acc.astype(np.float64)).astype(np.float32)
    return acc


@pytest.mark.parametrize("up,down,n", CASES)
def test_f32_emulation_is_under_the_bound(up, down, n):
    x, y, bound = case(up, down, n)
    assert R.worst(emulate(x, up, down), y, bound) <= 1


@pytest.mark.parametrize("wrong", R.WRONG)
def test_wrong_restatements_break_the_bound(wrong):
    broken = []
    for up, down, n in CASES:
        x, y, bound = case(up, down, n)
        if R.worst(R.resample(x, up, down, wrong=wrong)[0], y, bound, sides=2) > 1:
            broken.append((up, down, n))
    assert broken, "no case separates the wrong restatement %r" % wrong
    if wrong in ("phase", "clamp"):   # these are wrong at every ratio
        assert {c[:2] for c in broken} == set(R.RATIOS), (wrong, broken)
    if wrong == "no_pre":   # a whole `down` of zeros only moves rem by one: wrong where half % down != 0
        assert {c[:2] for c in broken} == {(u, d) for u, d in R.RATIOS if 10 * max(u, d) % d}, broken


def test_plan_and_paths():
    assert R.plan(441, 80) == dict(half=4410, pre=70, rem=56, n_taps=8821, J=21)
    assert R.plan(147, 320)["J"] == 46 and R.plan(1, 2)["J"] == 43
    assert 4 * 441 * 21 == 37044                       # the 16 kHz table: 37 KB of LDS
    want = {(11025, 5507): (True, False), (1, 20): (False, True), (800, 16000): (True, True)}
    for up, down in R.RATIOS:
        assert R.kernel_path(up, down) == want.get((up, down), (False, False)), (up, down)
    for up, down in R.RATIOS:
        n = R.n_in_past_three_runs(up, down)
        assert 3 * R.RUN < R.out_len(n, up, down) <= 3 * R.RUN + max(1, -(-up // down))
    assert R.out_len(R.n_in_past_three_runs(147, 80), 147, 80) == 3 * R.RUN + 1
    # workgroups of one CU: 8 unless LDS limits them (441/80: 37 KB table + span -> 4)
    assert [R.workgroups(u, d, 1) for u, d in [(147, 80), (441, 80), (11025, 5507), (1, 20), (800, 16000)]] \
        == [8, 4, 8, 8, 8]

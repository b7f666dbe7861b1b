"""nstl_resample_poly and nstl_peak_normalise (csrc/resample.hip) against
tests/resample_ref.py: every output element under the restatement's bound, at every ratio
of resample_ref.RATIOS (LDS table, table in global memory, samples in global memory,
both) and every length of resample_ref.lengths (1, 2, 37: shorter than one phase's taps;
1000; one output past three runs of a workgroup), and with the grid capped at one CU's
workgroups so that each workgroup walks three or more runs (the restaging of the input
span behind a barrier and the per-run base arithmetic), in all four instantiations.

The output buffer carries 16 NaN canaries after y[n_out - 1]; peak starts from garbage
(the entry point zeroes it) and must equal max |y| of the kernel's own output exactly;
two calls are bit-identical.

NSTL_RESAMPLE_PARITY_ERRORS_OUT=<file>: the worst err / bound of every case is appended
(profiles/resample_parity_errors.txt holds one such run)."""
import os

import numpy as np
import pytest
import torch

from tests import resample_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
_taps = {}


def record(name, ratio):
    line = "%-28s worst err/bound %.4f" % (name, ratio)
    print(line)
    path = os.environ.get("NSTL_RESAMPLE_PARITY_ERRORS_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def device_taps(up, down):
    if (up, down) not in _taps:
        _taps[up, down] = torch.tensor(R.taps(up, down).astype(np.float32), device=DEV)
    return _taps[up, down]


def run(x, up, down, peak=True):
    """One nstl_resample_poly call -> (y with its canaries, peak or None), on the CPU."""
    from neurosync_trainer_lite_amd import _hip as K
    n_out = K.resample_out_len(len(x), up, down)
    assert n_out == R.out_len(len(x), up, down)
    y = torch.full((n_out + 16,), NAN, dtype=torch.float32, device=DEV)
    pk = torch.full((1,), 3e38, dtype=torch.float32, device=DEV) if peak else None
    K.resample_poly(torch.tensor(x, device=DEV), up, down, device_taps(up, down), y[:n_out], peak=pk)
    torch.cuda.synchronize()
    return y.cpu().numpy(), (pk.cpu().numpy()[0] if peak else None)


def judge(name, x, up, down, ref, bound):
    n_out = len(ref)
    got, pk = run(x, up, down)
    assert np.isnan(got[n_out:]).all(), "samples after y[n_out - 1] were written"
    y = got[:n_out]
    ratio = R.worst(y, ref, bound)
    record(name, ratio)
    assert ratio <= 1, (name, ratio)
    assert pk.view(np.uint32) == np.max(np.abs(y)).view(np.uint32), "peak is not max |y| of the output"
    again, pk2 = run(x, up, down)
    assert np.array_equal(again[:n_out].view(np.uint32), y.view(np.uint32)) and pk2 == pk, "two calls differ"
    return y


@pytest.mark.parametrize("up,down,n", R.CASES)
def test_every_element_under_the_bound(up, down, n):
    x, ref, bound = R.case(up, down, n)
    judge("resample-%d/%d-n%d" % (up, down, n), x, up, down, ref, bound)


@pytest.mark.parametrize("up,down", R.RATIOS)
def test_unit_impulses_at_both_ends(up, down):
    """Sample 0 and the last sample: between them every tap a 1000-sample clip can reach is
    read once, alone in its sum, so a tap in the wrong place shows as itself."""
    x, ref, bound = R.case(up, down, 1000, impulse=True)
    y = judge("resample-%d/%d-impulses" % (up, down), x, up, down, ref, bound)
    assert np.all(y[bound == 0] == 0), "an output no term reaches must be exactly 0"


MANY_RUNS = [(147, 80, 25), (441, 80, 12), (11025, 5507, 25), (1, 20, 23), (800, 16000, 23)]


@pytest.mark.parametrize("up,down,runs", MANY_RUNS)
def test_a_workgroup_walks_several_runs(up, down, runs, monkeypatch):
    """NSTL_PERSIST_CUS=1 caps the grid at the workgroups of one CU (8, or 4 with the 37 KB
    table of 441/80), so a clip of `runs` + 1 runs sends every workgroup through its loop
    three times or more: run 2 and later restage the input span (after the barrier that
    lets the previous run's readers finish) and re-derive their phase and sample bases.
    Every element of every run is held to the same bound as in the one-run cases."""
    grid = R.workgroups(up, down, 1)
    n = R.n_in_past_runs(up, down, runs)
    assert R.out_len(n, up, down) > runs * R.RUN and runs + 1 >= 3 * grid, (grid, runs)
    x, ref, bound = R.case(up, down, n)
    monkeypatch.setenv("NSTL_PERSIST_CUS", "1")
    judge("resample-%d/%d-%druns-1cu" % (up, down, runs + 1), x, up, down, ref, bound)
    monkeypatch.delenv("NSTL_PERSIST_CUS")
    got, _ = run(x, up, down)             # the full grid on the same clip: the same bits
    monkeypatch.setenv("NSTL_PERSIST_CUS", "1")
    capped, _ = run(x, up, down)
    assert np.array_equal(got.view(np.uint32), capped.view(np.uint32))


def test_without_peak_the_output_is_the_same():
    x, ref, bound = R.case(147, 80, 1000)
    a, _ = run(x, 147, 80, peak=True)
    b, pk = run(x, 147, 80, peak=False)
    assert pk is None and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096 * 256 + 3])
def test_peak_normalise_is_numpys_division(n):
    """y / np.float32(m) bit for bit (IEEE division, not a reciprocal multiply); the last
    length is one grid stride and three elements."""
    from neurosync_trainer_lite_amd import _hip as K
    y = R.signal(n, n)
    y[0] = np.float32(1e-41)      # a subnormal quotient
    m = np.float32(np.max(np.abs(y)) if n > 1 else 3.0)
    buf = torch.full((n + 16,), NAN, dtype=torch.float32, device=DEV)
    buf[:n] = torch.tensor(y)
    K.peak_normalise(buf, torch.tensor([m], device=DEV), n=n)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.isnan(got[n:]).all()
    assert np.array_equal(got[:n].view(np.uint32), (y / np.float32(m)).view(np.uint32))


@pytest.mark.parametrize("peak", [0.0, -1.0])
def test_peak_normalise_leaves_a_silent_clip_alone(peak):
    from neurosync_trainer_lite_amd import _hip as K
    y = R.signal(1000, 5)
    buf = torch.tensor(y, device=DEV)
    K.peak_normalise(buf, torch.tensor([peak], dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), y.view(np.uint32))


def test_all_zero_clip_has_peak_zero():
    got, pk = run(np.zeros(1000, np.float32), 441, 80)
    assert pk == 0 and np.all(got[:R.out_len(1000, 441, 80)] == 0)


def test_rejections_launch_nothing():
    from neurosync_trainer_lite_amd import _hip as K
    x = torch.zeros(1000, device=DEV)
    y = torch.full((1838,), NAN, device=DEV)
    with pytest.raises(RuntimeError, match="n_taps"):
        K.resample_poly(x, 147, 80, device_taps(147, 160), y)
    with pytest.raises(RuntimeError, match="n_out"):
        K.resample_poly(x, 147, 80, device_taps(147, 80), y[:1837])
    torch.cuda.synchronize()
    assert torch.isnan(y).all()

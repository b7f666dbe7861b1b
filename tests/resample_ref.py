"""Float64 restatement of nstl_resample_poly (csrc/resample.hip) and the bound its f32
arithmetic is held to.

The rule (scipy.signal.resample_poly at its defaults): max_rate = max(up, down),
half = 10 max_rate, h = firwin(2 half + 1, 1 / max_rate, window=('kaiser', 5.0)) up;
pre = down - half % down zeros in front of h give hp; rem = (half + pre) // down;
n_out = ceil(n_in up / down); for output m, t0 = (m + rem) down and
    y[m] = sum of hp[k] x[(t0 - k) / up] over k == t0 (mod up), 0 <= k < len(hp),
terms whose sample index falls outside [0, n_in) dropped.

The bound, per output element, counted from the kernel's arithmetic: each tap is
rounded once to f32 (relative 2^-24) and each of the J = ceil(len(hp) / up) FMAs of the
chain rounds once (relative 2^-24 of a partial sum no larger than the sum of the
magnitudes), so the error is at most (J + 1) 2^-24 sum |hp[k]| |x[i]| to first order;
(J + 2) leaves room for the second-order terms.  A term that is dropped adds nothing to
either side, so an output no term reaches has bound 0: it must be exactly 0.

`wrong` selects a deliberately wrong restatement (tests/test_resample_ref.py shows that
each breaks the bound)."""
import numpy as np

U = 2.0 ** -24
RUN = 1024   # outputs per run of a workgroup (RS_RUN in csrc/resample.hip)
LDS_BYTES = 64 * 1024 - 64   # RS_LDS_BYTES

# (up, down): the source rate each stands for at a target of 88.2 kHz, and what it exercises
RATIOS = [
    (2, 1),         # 44.1 kHz: down = 1
    (4, 1),         # 22.05 kHz
    (147, 80),      # 48 kHz
    (441, 80),      # 16 kHz: the largest LDS table of the common rates
    (147, 160),     # 96 kHz
    (1, 2),         # 176.4 kHz: up = 1, pure decimation
    (147, 320),     # 192 kHz: 46 taps per phase
    (11025, 5507),  # 44,056 Hz: the table in global memory
    (1, 20),        # 1.764 MHz: the input span past LDS (samples from global memory)
    (800, 16000),   # both in global memory
]
WRONG = ("phase", "no_pre", "floor", "unscaled", "clamp")


def taps(up, down):
    """The prototype h in f64, scaled by up."""
    from scipy.signal import firwin
    max_rate = max(up, down)
    half = 10 * max_rate
    return firwin(2 * half + 1, 1.0 / max_rate, window=("kaiser", 5.0)) * up


def plan(up, down):
    half = 10 * max(up, down)
    pre = down - half % down
    rem = (half + pre) // down
    J = -(-(pre + 2 * half + 1) // up)
    return dict(half=half, pre=pre, rem=rem, n_taps=2 * half + 1, J=J)


def out_len(n_in, up, down):
    return -(-n_in * up // down)


def kernel_path(up, down):
    """(taps in global memory, samples in global memory): the launcher's rule."""
    J = plan(up, down)["J"]
    span = 4 * ((RUN - 1) * down // up + 2 + J)
    xg = span > LDS_BYTES
    tg = 4 * up * (J | 1) + (0 if xg else span) > LDS_BYTES
    return tg, xg


def workgroups(up, down, cus):
    """The launcher's grid for a clip of many runs on `cus` CUs: as many workgroups as fit
    a CU's 160 KB of LDS (8 at most) per CU; each walks runs blockIdx, + grid, ..."""
    J = plan(up, down)["J"]
    tg, xg = kernel_path(up, down)
    lds = (0 if tg else 4 * up * (J | 1)) + (0 if xg else 4 * ((RUN - 1) * down // up + 2 + J))
    return cus * max(1, min(8, 160 * 1024 // (lds + 64)))


def n_in_past_runs(up, down, runs):
    """The shortest input whose output is longer than `runs` runs."""
    n = (runs * RUN * down) // up + 1
    assert out_len(n, up, down) > runs * RUN >= out_len(n - 1, up, down)
    return n


def n_in_past_three_runs(up, down):
    """The shortest input whose output is longer than three runs: 3 RUN + 1 outputs where
    the ratio can land there (a fourth workgroup with one output), else the next length."""
    n = (3 * RUN * down) // up + 1
    assert out_len(n, up, down) > 3 * RUN >= out_len(n - 1, up, down)
    return n


def signal(n, seed):
    return (0.5 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def impulses(n):
    x = np.zeros(n, np.float32)
    x[0] = 1.0
    x[-1] = 1.0
    return x


def lengths(up, down):
    """1, 2, 37: shorter than one phase's taps, both edges meet inside one output."""
    return [1, 2, 37, 1000, n_in_past_three_runs(up, down)]


CASES = [(up, down, n) for up, down in RATIOS for n in lengths(up, down)]
_cache = {}


def case(up, down, n, impulse=False):
    """(x f32, y f64, bound f64) of one case, computed once per process."""
    key = (up, down, n, impulse)
    if key not in _cache:
        x = impulses(n) if impulse else signal(n, 1000 * up + down + n)
        _cache[key] = (x,) + resample(x, up, down)
    return _cache[key]


def resample(x, up, down, wrong=None):
    """(y, bound), f64 [n_out] each."""
    assert wrong is None or wrong in WRONG
    x = np.asarray(x, np.float64)
    n_in = len(x)
    P = plan(up, down)
    h = taps(up, down)
    if wrong == "unscaled":
        h = h / up
    pre = 0 if wrong == "no_pre" else P["pre"]
    rem = (P["half"] + pre) // down
    hp = np.concatenate([np.zeros(pre), h])
    n_out = n_in * up // down if wrong == "floor" else out_len(n_in, up, down)
    J = -(-len(hp) // up)
    j = np.arange(J, dtype=np.int64)
    y, mag = np.zeros(n_out), np.zeros(n_out)
    step = max(1, (1 << 21) // J)          # outputs per pass: the [step][J] temporaries stay small
    for lo in range(0, n_out, step):
        m = np.arange(lo, min(lo + step, n_out), dtype=np.int64)
        t0 = (m + rem) * down + (1 if wrong == "phase" else 0)
        p, q = t0 % up, t0 // up
        k = p[:, None] + j[None, :] * up
        i = q[:, None] - j[None, :]
        live = k < len(hp)
        if wrong == "clamp":
            i = np.clip(i, 0, n_in - 1)
        else:
            live &= (i >= 0) & (i < n_in)
        terms = np.where(live, hp[np.minimum(k, len(hp) - 1)] * x[np.clip(i, 0, n_in - 1)], 0.0)
        y[m] = terms.sum(axis=1)
        mag[m] = np.abs(terms).sum(axis=1)
    return y, (P["J"] + 2) * U * mag


def worst(got, ref, bound, sides=1):
    """max err / (sides x bound) over the elements (0 / 0 = 0); inf on a shape mismatch or
    a non-finite value."""
    got = np.asarray(got, np.float64)
    if got.shape != ref.shape or not np.isfinite(got).all():
        return float("inf")
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / (sides * bound))))

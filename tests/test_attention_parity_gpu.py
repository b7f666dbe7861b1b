"""Per-element float64 parity of every attention kernel (csrc/attention.hip,
csrc/attention_long.hip) against tests/attn_ref.py, and the exact dropout keep bits.

Every case is one nstl_attn_fwd + nstl_attn_bwd call, judged per element:
|got - ref| <= attn_ref.bound (its docstring derives it and gives the count c of bf16
roundings per kernel and output); no case is widened.  The launch counters pin the
kernel family each case means to reach.  Run with -s, the worst err / bound of every
case and output is printed (profiles/attention_parity_errors.txt is such a run).

Layout: q, k, v and dout each sit in a buffer of their own whose row stride is the
window + 8 (bf16) / + 4 (f32) elements, the padding columns NaN; o, dq, dk, dv, lse,
dsum, the keep words and dbias_part are pre-filled with NaN (the words with a fill
pattern), their padding columns and a tail behind them hold a sentinel that must
survive.  One case per kernel family keeps the packed qkv / dqkv layout.

RoPE^T: the pure bound holds for NSTL_ROPE_BWD=table.  The production default
recomputes cos / sin in the kernel (rope_tab_fast); one case per bf16 backward kernel
runs it under the table bound plus delta(t, i) (|e| + |o|) of the unrotated
reference pair, delta = FAST_A + FAST_B t inv_freq_i, measured on the GPU (see
FAST_A below; it cannot be derived: the accuracy of the hardware sin / cos / exp is
not documented)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import attn_ref as A

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from neurosync_trainer_lite_amd import _hip as K
    from neurosync_trainer_lite_amd.engine import rotation_tables

DEV = "cuda:0"
B, H, DH = 2, 3, 64
BF, F32 = torch.bfloat16, torch.float32
P_DROP = 0.3
SEED = (0x9E3779B9 << 32) | 0x00C0FFEE      # nonzero high word
SENT = 7.0                      # sentinel of the float buffers
SENT_W = 0x0123456789ABCDEF     # ... of the keep-bit words
FILL_W = 0x5A5A5A5A5A5A5A5A     # pre-fill of the words the call must write
NAN = float("nan")

# Fast RoPE^T: how far the recomputed cos / sin stray from the float64 values of the
# f32 tables, delta(t, i) <= FAST_A + FAST_B * t * inv_freq_i.  Measured on an MI355X
# by tools/attn_fast_rope_delta.py (profiles/attention_parity_errors.txt): a fast-mode
# streaming backward at T = 300 over 8192 heads, the stored (even, odd) pairs of dq
# and dk whose unrotated reference is at least half its row's maximum solved per
# (t, i), by least squares over the heads, for the implied (cos, sin).  Largest
# deviation 1.52e-4, at t inv_freq <= 1; nothing above it at larger angles, up to
# t inv_freq = 299, so the observed slope is 0.  A and B are twice these, and hold
# for T <= 300.  The solve works on bf16 outputs: its standard error is 1.9e-5, and
# with 512 heads every figure is four times larger, so they are the method's
# resolution, an upper limit of delta and not delta itself.
FAST_A, FAST_B = 3.1e-4, 0.0

# launch counters: (fwd_long, bwd_long, fwd_generic, bwd_generic, fwd, bwd_split, bwd_fused)
FUSED, SPLIT = (0, 0, 0, 0, 1, 0, 1), (0, 0, 0, 0, 1, 1, 0)
STREAMING, GENERIC = (1, 1, 0, 0, 0, 0, 0), (0, 0, 1, 1, 0, 0, 0)


def counts7(c):
    return (c["attn_fwd_long"], c["attn_bwd_long"], c["attn_fwd_generic"], c["attn_bwd_generic"], c["attn_fwd"],
            c["attn_bwd_split"], c["attn_bwd_fused"])


def heads(x, b, T, dh):
    """[b*T][H*dh] window -> [b][H][T][dh]"""
    return x.reshape(b, T, H, dh).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def inputs(dt, T, dh, b, scale=1.0):
    """q, k, v, dout [b*T][H*dh] of the case, compact, on the device."""
    def rnd(seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(b * T, H * dh, generator=g, dtype=torch.float64) * scale).to(dt).to(DEV)
    return tuple(rnd(1000 + s) for s in range(4))


@functools.lru_cache(maxsize=None)
def keep_of(bh, T, p):
    return A.keep(SEED, bh, T, p)


@functools.lru_cache(maxsize=None)
def forward_ref(dt, T, dh, b, p):
    """The float64 forward of a case's inputs, once per (shape, p)."""
    q, k, v, _ = (heads(x, b, T, dh) for x in inputs(dt, T, dh, b))
    return A.attn_fwd_ref(q, k, v, p, keep_of(b * H, T, p) if p else None)


def padded(x, dt):
    """x [M][D] in a buffer of its own, row stride D + 8 (bf16) / + 4 (f32), padding NaN."""
    M, D = x.shape
    buf = torch.full((M, D + (8 if dt == BF else 4)), NAN, dtype=dt, device=DEV)
    buf[:, :D] = x
    return buf


def guarded(rows, cols, pad, tail, dtype):
    """[rows + tail][cols + pad]: the [rows][cols] window NaN, everything else the sentinel."""
    t = torch.full((rows + tail, cols + pad), SENT, dtype=dtype, device=DEV)
    t[:rows, :cols] = NAN
    return t


def intact(name, t, rows, cols, what):
    assert (t[rows:].float() == SENT).all(), "%s: %s tail overwritten" % (what, name)
    assert (t[:rows, cols:].float() == SENT).all(), "%s: %s padding columns overwritten" % (what, name)
    assert not torch.isnan(t[:rows, :cols].float()).any(), "%s: %s NaN pre-fill left" % (what, name)


def run(dt, T, dh=DH, mode="none", b=B, flags=0, rope=(1, 1), packed=False, v_override=None):
    """One forward + backward.  mode: "none" (p = 0), "stored" (p = 0.3, keep words
    stored by the forward and read by the backward), "hashed" (p = 0.3, re-hashed)."""
    p = 0.0 if mode == "none" else P_DROP
    M, D, pad = b * T, H * dh, (8 if dt == BF else 4)
    q, k, v, do = inputs(dt, T, dh, b)
    if v_override is not None:
        v = v_override
    if packed:
        qkv = torch.cat([q, k, v], 1).contiguous()
        qb, kb, vb, ld_in = qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D
        dob, ld_do = do, D
        o = guarded(M, D, 0, 16, dt)
        dqkv = guarded(M, 3 * D, 0, 16, dt)
        dqb, dkb, dvb, ld_o, ld_d = dqkv, dqkv[:, D:], dqkv[:, 2 * D:], D, 3 * D
        outs = [("o", o, M, D), ("dqkv", dqkv, M, 3 * D)]
        win = dict(o=o[:M, :D], dq=dqkv[:M, :D], dk=dqkv[:M, D:2 * D], dv=dqkv[:M, 2 * D:])
    else:
        qb, kb, vb, dob = (padded(x, dt) for x in (q, k, v, do))
        ld_in = ld_do = ld_o = ld_d = D + pad
        o, dqb, dkb, dvb = (guarded(M, D, pad, 16, dt) for _ in range(4))
        outs = [("o", o, M, D), ("dq", dqb, M, D), ("dk", dkb, M, D), ("dv", dvb, M, D)]
        win = dict(o=o[:M, :D], dq=dqb[:M, :D], dk=dkb[:M, :D], dv=dvb[:M, :D])
    n = b * H * T
    lse, dsum = guarded(n, 1, 0, 64, F32), guarded(n, 1, 0, 64, F32)
    cs, sn = rotation_tables(T, dh, DEV)
    a = K.attn_args(K.dtype_code(dt), b, T, H, qb.data_ptr(), ld_in, kb.data_ptr(), ld_in, vb.data_ptr(), ld_in,
                    o.data_ptr(), ld_o, lse.data_ptr(), p, SEED, dh=dh, flags=flags)
    words = K.attn_mask_words(a)
    mask = None
    if mode == "stored" and words:
        mask = torch.full((words + 64,), SENT_W, dtype=torch.int64, device=DEV)
        mask[:words] = FILL_W
        a.mask_bits = mask.data_ptr()
    K.kernel_counts_reset()
    K.attn_fwd(a)
    a.dout, a.dout_ld = dob.data_ptr(), ld_do
    a.dq, a.dq_ld, a.dk, a.dk_ld, a.dv, a.dv_ld = dqb.data_ptr(), ld_d, dkb.data_ptr(), ld_d, dvb.data_ptr(), ld_d
    a.rope_cos, a.rope_sin, a.rope_q, a.rope_k = cs.data_ptr(), sn.data_ptr(), rope[0], rope[1]
    a.dsum = dsum.data_ptr()
    rows = K.attn_bias_rows(a)
    part = None
    if rows:
        part = guarded(rows, 3 * D, 0, 16, F32)
        a.dbias_part = part.data_ptr()
    K.attn_bwd(a)
    torch.cuda.synchronize()
    counts = counts7(K.kernel_counts())
    path = {FUSED: "fwd+fused", SPLIT: "fwd+split", STREAMING: "streaming", GENERIC: "generic"}.get(counts, str(counts))
    what = "%-9s %-4s T=%d dh=%d b=%d %s%s" % (path, "bf16" if dt == BF else "f32", T, dh, b, mode,
                                               " packed" if packed else "")
    for name, t, r, c in outs + [("lse", lse, n, 1)] + ([("dbias_part", part, rows, 3 * D)] if rows else []):
        intact(name, t, r, c, what)
    assert (dsum[n:] == SENT).all(), what + ": dsum tail overwritten"
    if counts[1] or counts[5]:  # the split and streaming dQ kernels fill it for their dK / dV kernels
        assert not torch.isnan(dsum[:n]).any(), what + ": dsum NaN pre-fill left"
    if mask is not None:
        assert (mask[words:] == SENT_W).all(), what + ": keep words tail overwritten"
    res = {nm: heads(x, b, T, dh) for nm, x in win.items()}
    res.update(lse=lse[:n, 0].reshape(b, H, T), dsum=dsum[:n, 0].reshape(b, H, T), counts=counts, words=words,
               mask=None if mask is None else mask[:words], rows=rows, part=None if part is None else part[:rows],
               flat={nm: x for nm, x in win.items()}, cs=cs, sn=sn, what=what, p=p, dt=dt, T=T, dh=dh, b=b,
               rope=rope, mode=mode)
    return res


def located(nm, ratio, idx, what):
    if len(idx) == 4:
        return "%s %s: worst err / bound %.3f at batch %d head %d row %d column %d" % ((what, nm, ratio) + idx)
    return "%s %s: worst err / bound %.3f at batch %d head %d row %d" % ((what, nm, ratio) + idx)


def fast_delta(T, dh):
    """[T][dh/2] f64: FAST_A + FAST_B * t * inv_freq_i"""
    t = torch.arange(T, dtype=torch.float64, device=DEV)[:, None]
    inv = torch.exp(-np.log(10000.0) * torch.arange(0, dh, 2, dtype=torch.float64, device=DEV) / dh)[None, :]
    return FAST_A + FAST_B * t * inv


def judge(r, c, fast=False):
    """Every output of run() per element against the float64 reference; prints and
    returns the worst ratios."""
    dt, T, dh, b, p, what = r["dt"], r["T"], r["dh"], r["b"], r["p"], r["what"]
    q, k, v, do = (heads(x, b, T, dh) for x in inputs(dt, T, dh, b))
    kp = keep_of(b * H, T, p) if p else None
    f = forward_ref(dt, T, dh, b, p)
    out = {"o": A.worst(r["o"], f["o"], A.bound(f["o"], f["mag_o"], dt, c, f["mag32_o"])),
           "lse": A.worst(r["lse"], f["lse"], A.lse_bound(f["lse_mag"]))}
    g = A.attn_bwd_ref(q, k, v, r["o"], None, do, p, kp, (r["cs"], r["sn"]) + r["rope"])
    plain = A.attn_bwd_ref(q, k, v, r["o"], None, do, p, kp, None) if fast else None
    for i, nm in enumerate(("dq", "dk", "dv")):
        bnd = A.bound(g[nm], g["mag_" + nm], dt, c, g["mag32_" + nm])
        if fast and nm != "dv" and r["rope"][i]:
            pair = plain[nm][..., 0::2].abs() + plain[nm][..., 1::2].abs()
            bnd = bnd + (fast_delta(T, dh) * pair).repeat_interleave(2, -1)
        out[nm] = A.worst(r[nm], g[nm], bnd)
    if r["counts"][1] or r["counts"][5]:
        out["dsum"] = A.worst(r["dsum"], g["dsum"], A.E32 * g["mag_dsum"])
    if r["part"] is not None:
        # row [b][128-row block]: the f64 column sums of that block's STORED dq | dk | dv
        D, nblk = H * dh, r["rows"] // b
        got = r["part"].double().reshape(b, nblk, 3 * D)
        stored = torch.cat([r["flat"][nm].double() for nm in ("dq", "dk", "dv")], 1).reshape(b, T, 3 * D)
        want, mag = torch.zeros_like(got), torch.zeros_like(got)
        for j in range(nblk):
            want[:, j] = stored[:, 128 * j:128 * (j + 1)].sum(1)
            mag[:, j] = stored[:, 128 * j:128 * (j + 1)].abs().sum(1)
        ratio, idx = A.worst(got, want, A.E32 * mag)
        assert ratio <= 1.0, "%s dbias_part: worst err / bound %.3f at batch %d block %d column %d" % ((what, ratio) + idx)
        out["dbias"] = (ratio, idx)
    env = {k: os.environ.get(k) for k in ("NSTL_ATTN_FWD", "NSTL_ATTN_BWD")}
    tag = what + "".join(" %s=%s" % (k[5:], v) for k, v in env.items() if v) + \
        (" rope %d%d" % r["rope"] if r["rope"] != (1, 1) else "") + (" fast-rope" if fast else "")
    print("\nPARITY %-66s c=%d " % (tag, c) + " ".join("%s %.4f" % (nm, x[0]) for nm, x in out.items()))
    for nm, (ratio, idx) in out.items():
        assert ratio <= 1.0, located(nm, ratio, idx, what)
    return out


def check_words(r):
    """The stored keep words, exactly: every bit in its tile, word and lane; bits of
    queries / keys past T are 0 and no word is left at its pre-fill."""
    bh, T = r["b"] * H, r["T"]
    nt = (T + 15) // 16
    assert r["words"] == bh * nt * nt * 4, r["what"]
    got = r["mask"].cpu().numpy().view(np.uint64)
    want = A.keep_words(keep_of(bh, T, r["p"]), T)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        w = int(bad[0])
        hd, qt, kt, kr = np.unravel_index(w, (bh, nt, nt, 4))
        raise AssertionError("%s: %d of %d keep words differ; first: head %d query tile %d key tile %d key %% 4 = %d: "
                             "%016x, want %016x" % (r["what"], bad.size, got.size, hd, qt, kt, kr, int(got[w]), int(want[w])))


def full_case(monkeypatch, dt, T, mode, counts, c, *, b=B, flags=0, dh=DH, env=(), rope=(1, 1), packed=False,
              rope_mode="table", twin=True):
    monkeypatch.setenv("NSTL_ROPE_BWD", rope_mode)
    for name, val in env:
        monkeypatch.setenv(name, val)
    r = run(dt, T, dh=dh, mode=mode, b=b, flags=flags, rope=rope, packed=packed)
    assert r["counts"] == counts, (r["what"], r["counts"])
    judge(r, c, fast=rope_mode == "fast")
    if r["mask"] is not None:
        check_words(r)
    if mode == "stored" and twin:
        # hashed and stored runs stay bit-equal
        h = run(dt, T, dh=dh, mode="hashed", b=b, flags=flags, rope=rope, packed=packed)
        for nm in ("o", "lse", "dq", "dk", "dv"):
            assert torch.equal(h[nm], r[nm]), "%s: stored vs hashed %s" % (r["what"], nm)
    return r


MODES = ["none", "stored", "hashed"]
ONESHOT = (("NSTL_ATTN_FWD", "oneshot"),)
SPLIT_ENV = (("NSTL_ATTN_BWD", "split"),)


# one-shot forward <bf16, NKT> (T = 128: NSTL_ATTN_FWD=oneshot) + fused backward <DM>
# (T = 128: TC = 128; otherwise runtime T)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [32, 64, 96, 128])
def test_oneshot_forward_fused_backward_bf16(T, mode, monkeypatch):
    full_case(monkeypatch, BF, T, mode, FUSED, 1, env=ONESHOT)


# persistent forward <MK> (stored: MK = true; hashed: p > 0 without mask_bits) + split backward at T = 128
@pytest.mark.parametrize("mode", MODES)
def test_persistent_forward_split_backward_bf16(mode, monkeypatch):
    full_case(monkeypatch, BF, 128, mode, SPLIT, 1, env=SPLIT_ENV)


def test_persistent_forward_equals_oneshot(monkeypatch):
    """The launch counters do not tell the two T = 128 forwards apart: both are judged
    per element above, and here they agree bit for bit, keep words included."""
    monkeypatch.setenv("NSTL_ATTN_FWD", "oneshot")
    one = run(BF, 128, mode="stored")
    monkeypatch.delenv("NSTL_ATTN_FWD")
    per = run(BF, 128, mode="stored")
    for nm in ("o", "lse", "mask"):
        assert torch.equal(one[nm], per[nm]), nm


# one-shot forward <bf16, NKT = 10 .. 16> + split backward <bf16, DM>
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [160, 192, 224, 256])
def test_oneshot_forward_split_backward_bf16(T, mode, monkeypatch):
    full_case(monkeypatch, BF, T, mode, SPLIT, 1)


# one-shot forward <float, NKT> + split backward <float, DM>
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [32, 64, 96, 128])
def test_oneshot_forward_split_backward_f32(T, mode, monkeypatch):
    full_case(monkeypatch, F32, T, mode, SPLIT, 0)


# streaming forward, dQ, dK / dV: whole tiles without the flag, ragged T with it
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [288, 320, 7, 100, 257, 300])
def test_streaming_bf16(T, mode, monkeypatch):
    full_case(monkeypatch, BF, T, mode, STREAMING, 1, flags=0 if T % 32 == 0 else K.ATTN_RAGGED_OK)


# one batch: rows past T are not another batch's rows, an overrun lands on the sentinel
@pytest.mark.parametrize("T", [7, 100, 257, 300])
def test_streaming_ragged_one_batch(T, monkeypatch):
    full_case(monkeypatch, BF, T, "stored", STREAMING, 1, b=1, flags=K.ATTN_RAGGED_OK)


# generic kernels: no bf16 rounding between the scores and the outputs (c = 0)
@pytest.mark.parametrize("mode", ["none", "hashed"])
@pytest.mark.parametrize("dt,T,dh", [(F32, 7, 24), (F32, 48, 64), (BF, 40, 64), (BF, 100, 128), (BF, 300, 64)])
def test_generic(dt, T, dh, mode, monkeypatch):
    full_case(monkeypatch, dt, T, mode, GENERIC, 0, dh=dh)


# today's layout: packed qkv [M][3D], o [M][D], dqkv [M][3D]
@pytest.mark.parametrize("dt,T,counts,c,flags", [(BF, 64, FUSED, 1, 0), (BF, 192, SPLIT, 1, 0), (F32, 96, SPLIT, 0, 0),
                                                 (BF, 300, STREAMING, 1, 1), (BF, 40, GENERIC, 0, 0)])
def test_packed_layout(dt, T, counts, c, flags, monkeypatch):
    full_case(monkeypatch, dt, T, "stored" if counts != GENERIC else "hashed", counts, c, flags=flags, packed=True)


@pytest.mark.parametrize("rope", [(1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("T,counts,flags", [(96, FUSED, 0), (160, SPLIT, 0), (300, STREAMING, 1)])
def test_rope_selection(T, counts, flags, rope, monkeypatch):
    full_case(monkeypatch, BF, T, "hashed", counts, 1, flags=flags, rope=rope)


# the production default: cos / sin recomputed in the kernel
@pytest.mark.parametrize("T,counts,flags", [(96, FUSED, 0), (128, FUSED, 0), (160, SPLIT, 0), (300, STREAMING, 1)])
def test_fast_rope(T, counts, flags, monkeypatch):
    full_case(monkeypatch, BF, T, "stored", counts, 1, flags=flags, rope_mode="fast", twin=False)


@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("T", [7, 40, 104])
def test_generic_keep_pattern_exact(dt, T, monkeypatch):
    """The generic kernels store no keep words: V = [I | 0] (dh = T rounded up to 8)
    reveals P keep / (1 - p) through O, which is nonzero exactly where the element is
    kept, wherever P itself is not 0."""
    monkeypatch.setenv("NSTL_ROPE_BWD", "table")
    dh = (T + 7) // 8 * 8
    eye = torch.zeros(T, dh, dtype=dt, device=DEV)
    eye[:, :T] = torch.eye(T, dtype=dt, device=DEV)
    vI = eye.repeat(B, H)  # [B*T][H*dh]: V[b, t, h, :] = e_t
    r = run(dt, T, dh=dh, mode="hashed", v_override=vI)
    assert r["counts"] == GENERIC, r["counts"]
    Pd = r["o"].double()[..., :T].reshape(B * H, T, T)
    q, k, _, _ = (heads(x, B, T, dh).double() for x in inputs(dt, T, dh, B))
    P = torch.softmax((q @ k.transpose(-1, -2)) * dh ** -0.5, -1).reshape(B * H, T, T)
    live = P > 1e-30  # far above the f32 underflow of the kernel's own P
    assert live.float().mean().item() > 0.99
    want = torch.from_numpy(keep_of(B * H, T, P_DROP)).to(DEV)
    diff = ((Pd != 0) != want) & live
    assert not diff.any(), "%d keep decisions differ, first at (head, query, key) %s" % (
        int(diff.sum()), tuple(int(x) for x in diff.nonzero()[0]))

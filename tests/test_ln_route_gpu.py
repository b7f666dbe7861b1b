"""_hip.ln_args / ln_set against a hand-filled LnArgs on the MI355X: one forward and one
backward each way on the same inputs, every output compared bit for bit.  It is the same
library and the same kernel, so any difference is a binding error (an operand pointed at
the wrong tensor, a stride or a scalar not carried over).  One width per kernel family
and per lane group (the table above nstl_ln_args in include/nstl.h), 13 rows, two masks
at p = 0.3, the rope rotation, and the e4m3 side copy where the width has one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from neurosync_trainer_lite_amd import _hip as K
    from neurosync_trainer_lite_amd.engine import FP8_WIDTHS, rotation_tables

DEV = "cuda:0"
F32, BF16, E4 = torch.float32, torch.bfloat16, torch.float8_e4m3fn
ROWS, P, EPS, ROPE_T = 13, 0.3, 1e-5, 5
SEEDS = ((0x9E3779B9 << 32) | 0x01234567, (0x7F4A7C15 << 32) | 0x89ABCDEF)
BITS = {4: torch.int32, 2: torch.int16, 1: torch.uint8}


def rnd(*shape, dtype=F32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype).to(DEV)


def nans(*shape, dtype=F32):
    if dtype == E4:  # both e4m3 NaN encodings have the low seven bits set
        return torch.full(shape, 0x7F, dtype=torch.uint8, device=DEV).view(E4)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def isnan(t):
    return (t.view(torch.uint8) & 0x7F) == 0x7F if t.dtype == E4 else torch.isnan(t)


def outputs(dt, D, n_part, q8):
    """NaN-prefilled, one spare row each."""
    o = dict(s_out=nans(ROWS + 1, D, dtype=dt), out=nans(ROWS + 1, D, dtype=dt), rot_out=nans(ROWS + 1, D, dtype=dt),
             mean=nans(ROWS + 1), rstd=nans(ROWS + 1), ds=nans(ROWS + 1, D), dbranch=nans(ROWS + 1, D, dtype=dt),
             dgamma_part=nans(n_part + 1, D), dbeta_part=nans(n_part + 1, D), dbranch_part=nans(n_part + 1, D))
    if q8:  # forward and backward copies, rows D + 16 apart
        for k in ("q8_f", "q8_b"):
            o[k] = nans(ROWS + 1, D + 16, dtype=E4)
            o[k + "_scale"] = nans(ROWS + 1)
    return o


def run_set(dt, D, n_part, inp, rope, o, q8):
    a = K.ln_args(K.dtype_code(dt), ROWS, D, 2, P, *SEEDS, eps=EPS, n_part=n_part)
    K.ln_set(a, rope_T=ROPE_T, x=inp["x"], y=inp["y"], gamma=inp["gamma"], beta=inp["beta"], s_out=o["s_out"], out=o["out"],
             mean=o["mean"], rstd=o["rstd"], rot_out=o["rot_out"], rope_cos=rope[0], rope_sin=rope[1])
    if q8:
        K.ln_set(a, q8=o["q8_f"][:, :D], q8_scale=o["q8_f_scale"])
    route = [K.ln_route(a)]
    K.ln_fwd(a)
    K.ln_set(a, s_in=o["s_out"], dout=inp["dout"], ds=o["ds"], dbranch=o["dbranch"], dout2=inp["dout2"],
             dgamma_part=o["dgamma_part"], dbeta_part=o["dbeta_part"], dbranch_part=o["dbranch_part"])
    if q8:
        K.ln_set(a, q8=o["q8_b"][:, :D], q8_scale=o["q8_b_scale"])
    route.append(K.ln_route(a, backward=True))
    K.ln_bwd(a)
    return route


def run_hand(dt, D, n_part, inp, rope, o, q8):
    a = K.LnArgs()
    a.dtype, a.rows, a.D = K.dtype_code(dt), ROWS, D
    a.x, a.y = inp["x"].data_ptr(), inp["y"].data_ptr()
    a.n_masks, a.p_drop, a.seed1, a.seed2 = 2, P, SEEDS[0], SEEDS[1]
    a.gamma, a.beta, a.eps = inp["gamma"].data_ptr(), inp["beta"].data_ptr(), EPS
    a.s_out, a.out, a.mean, a.rstd = o["s_out"].data_ptr(), o["out"].data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr()
    a.rot_out, a.rope_cos, a.rope_sin, a.rope_T = o["rot_out"].data_ptr(), rope[0].data_ptr(), rope[1].data_ptr(), ROPE_T
    if q8:
        a.q8, a.ldq8, a.q8_scale = o["q8_f"].data_ptr(), D + 16, o["q8_f_scale"].data_ptr()
    route = [K.ln_route(a)]
    K.ln_fwd(a)
    a.s_in, a.dout, a.ds, a.dbranch = o["s_out"].data_ptr(), inp["dout"].data_ptr(), o["ds"].data_ptr(), o["dbranch"].data_ptr()
    a.dout2 = inp["dout2"].data_ptr()
    a.dgamma_part, a.dbeta_part, a.n_part = o["dgamma_part"].data_ptr(), o["dbeta_part"].data_ptr(), n_part
    a.dbranch_part = o["dbranch_part"].data_ptr()
    if q8:
        a.q8, a.q8_scale = o["q8_b"].data_ptr(), o["q8_b_scale"].data_ptr()
    route.append(K.ln_route(a, backward=True))
    K.ln_bwd(a)
    return route


@pytest.mark.parametrize("n_part", [1, 2])
@pytest.mark.parametrize("D", [128, 256, 384, 768, 1536])
@pytest.mark.parametrize("dt", [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")])
def test_ln_set_call_equals_the_hand_filled_call(dt, D, n_part):
    inp = dict(x=rnd(ROWS, D, dtype=dt, seed=1), y=rnd(ROWS, D, dtype=dt, seed=2), gamma=1 + 0.1 * rnd(D, seed=3),
               beta=0.1 * rnd(D, seed=4), dout=rnd(ROWS, D, seed=5), dout2=rnd(ROWS, D, dtype=dt, seed=6))
    rope = rotation_tables(ROPE_T, D, DEV)
    q8 = dt == BF16 and D in FP8_WIDTHS
    o_set, o_hand = outputs(dt, D, n_part, q8), outputs(dt, D, n_part, q8)
    r_set = run_set(dt, D, n_part, inp, rope, o_set, q8)
    r_hand = run_hand(dt, D, n_part, inp, rope, o_hand, q8)
    torch.cuda.synchronize()
    assert r_set == r_hand and not any(r.startswith("rejected") for r in r_set), (r_set, r_hand)
    assert all(r.endswith(" q8") for r in r_set) == q8, r_set
    for name, t in o_set.items():
        n = n_part if name.endswith("_part") else ROWS
        written = t[:n, :D] if name in ("q8_f", "q8_b") else t[:n]
        assert not isnan(written).any(), name + ": NaN in (or no write to) a written row"
        assert isnan(t[n:]).all(), name + ": wrote past its extent"
        if name in ("q8_f", "q8_b"):
            assert isnan(t[:, D:]).all(), name + ": wrote between the rows"
        bits = BITS[t.element_size()]
        assert torch.equal(t.view(bits), o_hand[name].view(bits)), name + ": ln_set and the hand-filled call differ"

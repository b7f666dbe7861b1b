"""A whole training step with dropout ON against the float64 CPU oracle, the oracle
taking the engine's own masks as input (oracle/model_ref.py `masks`, built by
tests/step_ref.site_masks from the forward's base seed and the three keep restatements
that already judge the kernels).  What only a whole step can show is judged here: which
site seed each forward and backward launch gets, the scale of the stacked masks, the
per-layer keep-word and ReLU-bit buffers, the saved p / seed, the rank salt.
tests/test_step_ref.py proves the reference on the CPU and shows that six such
mistakes move a gradient by more than any gate below.

One step: torch.manual_seed, train(), forward, loss, backward, base seed from
engine.saved["seed"], masks, OracleTrainer(float64).step(masks=...), then loss,
prediction, every gradient, the clip norm, and after opt.step(max_norm=2.0) every
parameter.  Error of a tensor: ||a - b|| / ||b|| (test_model_gpu.rel).

Gates.
  fp32 (test_model_gpu.test_fp32_step_matches_reference's): worst gradient 1e-4,
    prediction rtol = atol = 1e-4, loss 1e-5, clip norm 1e-4.
  bf16: (1) the project's caps (test_bf16_step_tracks_oracle): 0.1 per gradient, 3e-2
    prediction, 2e-2 loss; the clip norm 0.1 (||g|| moves by at most ||dg||).
    (2) each figure's dropout-on error is at most max(FLOOR, K_RATIO x its error in the
    same config and weights with dropout 0 against the unmasked oracle).  FLOOR is one
    bf16 ulp, 2^-7: no bf16 pipeline promises a tensor less, and a ratio to an error
    below it is noise.  K_RATIO is twice the worst on/off ratio measured on an MI355X
    over every figure of every bf16 case here whose dropout-on error exceeds FLOOR
    (profiles/dropout_step_parity_errors.txt).  The gate of a figure is
    min(cap, max(FLOOR, K_RATIO x off)), so none exceeds 0.1, which every mutant of
    tests/test_step_ref.py clears.
  parameters after the step, both modes: 2 x lr per element (test_model_gpu: Adam's
    first step moves an element by lr g / (|g| + eps), so one whose gradient is ~0 may
    legitimately land on the other side), and lr / 2 on the mean of a tensor.

Shapes are the smallest that enter each path (asserted by the launch counters):
  fp32  D128 H2 L2 B2 T32   one-shot f32 attention forward, split backward (dh 64)
  fp32  D128 H4 L1 B3 T40   generic attention (dh 32, ragged T)
  fp32  D128 H2 L1 B2 T160  generic attention (f32 past T = 128)
  bf16  D256 H4 L2 B16 T128 2048 rows: FFN1 is 32 tiles of 256^2, the GEMMs that store
                            the ReLU bits; one-shot attention with stored keep words,
                            fused backward; two layers
  bf16  D256 H4 L1 B2 T288  streaming attention with keep words
  bf16  D256 H4 L1 B2 T300  the same, ragged
  bf16  D256 H2 L1 B2 T64   head_dim 128 streaming
  bf16  D256 H4 L2 B4 T64 p 0.1   256 rows, FFN1 4 tiles: no side outputs (no stored ReLU
                            bits, no colsum_part: the dReLU from the saved hidden, the bias
                            gradient by nstl_colsum), at a second p.  At 256 rows the
                            4-wave kernel still runs the whole-tile GEMMs, so
  bf16  D256 H4 L2 B3 T64 p 0.1   192 rows: every GEMM on the 128 x 128 kernel"""
import numpy as np
import pytest
import torch

from oracle import model_ref
from tests import attn_ref as A
from tests import step_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FLOOR = 2.0 ** -7
# twice 1.594, the worst measured (decoder layer 0 norm2.weight of the accumulation case)
K_RATIO = 3.2
CAPS = {"grad": 0.1, "pred": 3e-2, "loss": 2e-2, "norm": 0.1}

FP32_CASES = [(128, 2, 2, 2, 32, 0.3), (128, 4, 1, 3, 40, 0.3), (128, 2, 1, 2, 160, 0.3)]
BF16_CASES = [(256, 4, 2, 16, 128, 0.3), (256, 4, 1, 2, 288, 0.3), (256, 4, 1, 2, 300, 0.3), (256, 2, 1, 2, 64, 0.3),
              (256, 4, 2, 4, 64, 0.1), (256, 4, 2, 3, 64, 0.1)]
LIFE = (256, 4, 1, 2, 64, 0.3)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def tag(case):
    return "D%d H%d L%d B%d T%d p%.1f" % case


def make(case, amp, dropout):
    from neurosync_trainer_lite_amd.config import training_config
    from neurosync_trainer_lite_amd.utils.model_utils import build_model, prepare_training_components
    D, H, L = case[:3]
    cfg = dict(training_config)
    cfg.update(hidden_dim=D, num_heads=H, n_layers=L, dropout=dropout, use_amp=amp)
    model = build_model(cfg, DEV)
    params = model_ref.seeded_params(model_ref.param_shapes(256, D, L, 61), 41)
    model.load_state_dict(params, strict=True)
    crit, opt, _ = prepare_training_components(cfg, model)
    return cfg, model, crit, opt, params


def batch(case, seed):
    B, T = case[3], case[4]
    rng = np.random.default_rng(seed)
    src = torch.tensor(rng.standard_normal((B, T, 256)).astype(np.float32))
    trg = torch.tensor((rng.standard_normal((B, T, 61)) * 20).astype(np.float32))
    return src, trg


def oracle_of(case, params, cfg):
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    return model_ref.OracleTrainer(params, case[1], lr=cfg["learning_rate"], weight_decay=cfg["weight_decay"],
                                   dtype=torch.float64)


def masks_of(case, seed, p):
    D, H, L, B, T = case[:5]
    return S.site_masks(seed, B, T, D, H, L, p) if p > 0 else None


def one_step(case, amp, dropout, torch_seed=7, salt=0, after_forward=None):
    """The engine's step and the oracle's on the same weights, batch and masks.
    Returns (errors {figure: rel}, extras)."""
    from neurosync_trainer_lite_amd import _hip as K
    cfg, model, crit, opt, params = make(case, amp, dropout)
    eng = model.engine(torch.device(DEV))
    eng.seed_salt = salt
    src, trg = batch(case, 3)
    torch.manual_seed(torch_seed)
    model.train()
    opt.zero_grad()
    K.kernel_counts_reset()
    pred = model(src.to(DEV))
    if after_forward is not None:
        torch.cuda.synchronize()
        after_forward(eng)
    loss = crit(pred, trg.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    counts = K.kernel_counts()
    seed = eng.saved["seed"]
    assert eng.saved["p"] == dropout and (seed != 0) == (dropout > 0)
    named = dict(model.named_parameters())
    grads = {k: named[k].grad.detach().double().cpu().clone() for k in params}
    oracle = oracle_of(case, params, cfg)
    o_loss, o_norm, o_pred = oracle.step(src.double(), trg.double(), masks=masks_of(case, seed, dropout))
    opt.step(max_norm=2.0)
    torch.cuda.synchronize()
    errs = {"loss": abs(loss.item() - o_loss.item()) / abs(o_loss.item()), "pred": rel(pred.detach(), o_pred),
            "norm": abs(opt.last_norm.item() - o_norm.item()) / o_norm.item()}
    errs.update({k: rel(grads[k], oracle.last_grads[k]) for k in params})
    # over the tensors: worst element past 2 lr + the f32 storage rounding of the parameter; worst mean
    lr = cfg["learning_rate"]
    diff = {k: (named[k].detach().double().cpu() - oracle.p[k].detach()).abs() for k in params}
    step_err = max((diff[k].max() - 2.0 ** -23 * oracle.p[k].detach().abs().max()).item() for k in params)
    mean_step = max(d.mean().item() for d in diff.values())
    return errs, dict(pred=pred.detach().cpu(), o_pred=o_pred, counts=counts, seed=seed, eng=eng, step_err=step_err,
                      mean_step=mean_step, lr=lr, o_norm=o_norm.item(), loss=loss.item())


def check_update(x):
    """Parameters after clip + Adam: 2 lr per element (module docstring) plus one f32 ulp
    of the parameter as stored (already subtracted in step_err), and lr / 2 on a
    tensor's mean: an update that did not happen, or happened twice, is off by lr on
    nearly every element, a correct one only where the gradient's sign differs."""
    assert x["step_err"] <= 2 * x["lr"], x["step_err"]
    assert x["mean_step"] <= 0.5 * x["lr"], x["mean_step"]


def kind(name):
    return name if name in ("loss", "pred", "norm") else "grad"


def show(what, case, errs, off=None):
    print("\n%s %s" % (what, tag(case)))
    for k, e in errs.items():
        if off is None:
            print("  %-62s %.3e" % (k, e))
        else:
            print("  %-62s on %.3e off %.3e ratio %6.2f%s" % (k, e, off[k], e / max(off[k], 1e-30),
                                                           "" if e > FLOOR else "  (below FLOOR)"))
    if off is not None:
        over = [errs[k] / max(off[k], 1e-30) for k in errs if errs[k] > FLOOR]
        print("  worst on/off ratio among figures above FLOOR: %s" % ("%.3f" % max(over) if over else "none above"))


def gate_bf16(what, case, errs, off):
    """Both parts of the bf16 gate, every figure; prints before it asserts."""
    show(what, case, errs, off)
    bad = {}
    for k, e in errs.items():
        cap = CAPS[kind(k)]
        g = min(cap, max(FLOOR, K_RATIO * off[k]))
        if not e < cap or not e <= g:
            bad[k] = (e, off[k], g)
    assert not bad, bad


_OFF = {}


def off_errors(case):
    """The same config and weights with dropout 0 against the unmasked oracle (once per
    config: the lifecycle tests share theirs)."""
    if case not in _OFF:
        errs, x = one_step(case, True, 0.0)
        _OFF[case] = errs
    return _OFF[case]


def check_counts(case, amp, c, eng):
    D, H, L, B, T, p = case
    n = 3 * L  # encoder self-, decoder self- and cross-attention of every layer
    dh = D // H
    att = {k: v for k, v in c.items() if k.startswith("attn")}
    print("  launches: %s" % {k: v for k, v in c.items() if v})
    if not amp:
        if dh == 64 and T % 32 == 0 and T <= 128:
            assert att["attn_fwd"] == n and att["attn_bwd_split"] == n and att["attn_fwd_generic"] == 0, att
        else:
            assert att["attn_fwd_generic"] == n and att["attn_bwd_generic"] == n and att["attn_fwd"] == 0, att
        return
    if dh == 128 or T > 256 or T % 32:
        assert att["attn_fwd_long"] == n and att["attn_bwd_long"] == n, att
        assert att["attn_fwd"] == att["attn_fwd_generic"] == att["attn_bwd_generic"] == 0, att
    else:
        assert att["attn_fwd"] == n and att["attn_bwd_fused"] == n and att["attn_fwd_generic"] == 0, att
    bb = eng.saved["bb"]
    side = all(bb.e_rmask_ok) and all(bb.d_rmask_ok)
    if B * T >= 2048:
        # FFN1 is ceil(M/256) x ceil(4D/256) >= 32 tiles: the 256-wide kernels with the stored ReLU bits
        assert side and c["gemm_ring"] + c["gemm4"] > 0, (bb.e_rmask_ok, bb.d_rmask_ok, c)
    else:
        assert not any(bb.e_rmask_ok) and not any(bb.d_rmask_ok), (bb.e_rmask_ok, bb.d_rmask_ok)
    if B * T < 256:
        assert c["gemm128"] > 0 and c["gemm4"] == c["gemm_ring"] == c["gemm_group"] == 0, c


# ------------------------------------------------------------------------------ fp32
@pytest.mark.parametrize("case", FP32_CASES, ids=tag)
def test_fp32_dropout_step_matches_masked_oracle(case):
    errs, x = one_step(case, False, case[5])
    show("fp32", case, errs)
    check_counts(case, False, x["counts"], x["eng"])
    print("  parameters after the step: worst |diff| %.3e, worst mean %.3e (lr %.1e)" % (x["step_err"], x["mean_step"], x["lr"]))
    grads = {k: e for k, e in errs.items() if kind(k) == "grad"}
    worst = max(grads, key=grads.get)
    assert grads[worst] < 1e-4, (worst, grads[worst])
    np.testing.assert_allclose(x["pred"].numpy(), x["o_pred"].numpy(), rtol=1e-4, atol=1e-4)
    assert errs["loss"] < 1e-5, errs["loss"]
    assert errs["norm"] < 1e-4, errs["norm"]
    check_update(x)


# ------------------------------------------------------------------------------ bf16
def relu_bits(words, M, N):
    """bool [M][N] of the stored ReLU keep&positive bits (gemm.hip relu_mask_index):
    word ((row >> 6) * 8 + (row & 7)) * ceil(N / 8) + col / 8, byte (row & 63) >> 3,
    bit col & 7."""
    rb, cg = (M + 63) // 64, (N + 7) // 8
    w = np.ascontiguousarray(words[:rb * 8 * cg]).view(np.uint8).reshape(rb, 8, cg, 8)   # [rb][r0][cg][byte]
    bits = np.unpackbits(w[..., None], axis=-1, bitorder="little")                       # [rb][r0][cg][byte][bit]
    return bits.transpose(0, 3, 1, 2, 4).reshape(rb * 64, cg * 8)[:M, :N].astype(bool)


def check_stored_bits(case, eng):
    """After the forward: every layer's attention keep words equal the reference's of
    that layer's attn / xattn seed, bit for bit, and no stored ReLU bit is set where
    that layer's ffn mask drops."""
    from neurosync_trainer_lite_amd.engine import _seed
    D, H, L, B, T, p = case
    bb, base = eng.saved["bb"], eng.saved["seed"]
    nt = (T + 15) // 16
    nw = B * H * nt * nt * 4
    for l in range(L):
        for enc, buf, site in ((True, bb.e_mask, "attn"), (False, bb.d_mask, "attn"), (False, bb.d_maskc, "xattn")):
            got = buf[l][:nw].cpu().numpy().view(np.uint64)
            want = A.keep_words(A.keep(_seed(base, enc, l, site), B * H, T, p), T)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s layer %d %s: %d of %d keep words differ, first %d: %016x want %016x" % (
                "encoder" if enc else "decoder", l, site, bad.size, nw, bad[0], int(got[bad[0]]), int(want[bad[0]]))
        for enc, buf, ok in ((True, bb.e_rmask, bb.e_rmask_ok), (False, bb.d_rmask, bb.d_rmask_ok)):
            assert ok[l]
            stored = relu_bits(buf[l].cpu().numpy(), B * T, 4 * D)
            keep = S.site_keep(_seed(base, enc, l, "ffn"), "ffn", B, T, D, H, p).reshape(B * T, 4 * D).numpy()
            assert not (stored & ~keep).any(), "%s layer %d: %d ReLU bits set where the ffn mask drops" % (
                "encoder" if enc else "decoder", l, int((stored & ~keep).sum()))
            # about half of the kept pre-activations are positive: the bits are this layer's, not left-over zeros
            assert 0.25 < stored.sum() / keep.sum() < 0.75, stored.sum() / keep.sum()


@pytest.mark.parametrize("case", BF16_CASES, ids=tag)
def test_bf16_dropout_step_matches_masked_oracle(case):
    first = case == BF16_CASES[0]
    errs, x = one_step(case, True, case[5], after_forward=(lambda eng: check_stored_bits(case, eng)) if first else None)
    off = off_errors(case)
    print("  parameters after the step: worst |diff| %.3e, worst mean %.3e (lr %.1e)" % (x["step_err"], x["mean_step"], x["lr"]))
    check_counts(case, True, x["counts"], x["eng"])
    gate_bf16("bf16", case, errs, off)
    check_update(x)


# ------------------------------------------------------------------------- lifecycle
def test_eval_forward_between_forward_and_backward_changes_nothing():
    """saved["p"] / saved["seed"]: an eval forward of another batch between a training
    forward and its backward leaves the gradients bitwise as without it."""
    cfg, model, crit, opt, params = make(LIFE, True, LIFE[5])
    src, trg = (t.to(DEV) for t in batch(LIFE, 3))
    other = batch(LIFE, 4)[0].to(DEV)
    got = []
    for interleave in (False, True):
        torch.manual_seed(7)
        model.train()
        opt.zero_grad()
        loss = crit(model(src), trg)
        if interleave:
            model.eval()
            with torch.no_grad():
                model(other)
            model.train()
            eng = model.engine(torch.device(DEV))
            assert eng.p == 0.0 and eng.saved["p"] == LIFE[5]  # the eval forward did change the live state
        loss.backward()
        torch.cuda.synchronize()
        got.append({k: p.grad.detach().clone() for k, p in model.named_parameters()})
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), k
    assert all(g.abs().sum() > 0 for g in got[0].values())


def accumulate(dropout):
    """Two micro-batches under two torch seeds into the same gradients, against the sum
    of the two (masked) oracle gradients."""
    cfg, model, crit, opt, params = make(LIFE, True, dropout)
    eng = model.engine(torch.device(DEV))
    model.train()
    opt.zero_grad()
    want, seeds = None, []
    for i, torch_seed in enumerate((7, 8)):
        src, trg = batch(LIFE, 3 + i)
        torch.manual_seed(torch_seed)
        crit(model(src.to(DEV)), trg.to(DEV)).backward()
        seeds.append(eng.saved["seed"])
        oracle = oracle_of(LIFE, params, cfg)
        oracle.step(src.double(), trg.double(), masks=masks_of(LIFE, seeds[-1], dropout))
        want = oracle.last_grads if want is None else {k: want[k] + oracle.last_grads[k] for k in want}
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    return {k: rel(named[k].grad, want[k]) for k in params}, seeds


def test_accumulated_micro_batches_match_the_sum_of_masked_oracles():
    errs, seeds = accumulate(LIFE[5])
    assert seeds[0] != seeds[1]
    off, _ = accumulate(0.0)
    gate_bf16("bf16 accumulation", LIFE, errs, off)


def test_rank_salt_changes_masks_and_step_still_matches():
    torch.manual_seed(7)
    draw = int(torch.randint(0, 2 ** 62, (1,)).item())
    errs, x = one_step(LIFE, True, LIFE[5], torch_seed=7, salt=1)
    assert x["seed"] == S.salted_seed(draw, 1) != S.salted_seed(draw, 0)
    D, H, L, B, T, p = LIFE
    m0, m1 = S.site_masks(S.salted_seed(draw, 0), B, T, D, H, L, p), S.site_masks(x["seed"], B, T, D, H, L, p)
    assert all(not torch.equal(m0[k], m1[k]) for k in m0)
    gate_bf16("bf16 seed_salt 1", LIFE, errs, off_errors(LIFE))

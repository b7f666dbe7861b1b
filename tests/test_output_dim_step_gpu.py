"""Whole training steps, inference, validation and a checkpoint round trip at
output_dim 68 and 128 (the wide output head: pred / dpred rows padded to 128, the
fused loss on its [128][129] tile), against the CPU oracle in float64, in the scheme
of tests/test_model_widths_gpu.py: seeded parameters from model_ref.param_shapes(256,
D, 1, out), dropout 0, one layer, the batch from default_rng(seed), targets scaled by
20.

fp32 mode: pred rel < 1e-4, loss within 1e-4, worst parameter gradient rel < 1e-4 (the
project's fp32 figures).  The test first asserts on the oracle alone that every FFN
pre-activation is at least 2 x 2^-24 x (sum_k |w_k x_k| + |b|) from zero (the reason
is in tests/test_model_widths_gpu.py); batch seed 3 gives margins 7.95 and 9.70 at the
two shapes (7.80 at the first with another host's float64 matrix products).
bf16: pred rel < 3e-2, loss within 2e-2; each parameter's gradient within max(0.1,
2 x the error of the same-named parameter in the same shape at output_dim = 61), the
present width being the yardstick, never the one under test; loss_wide counts one
launch per step; no generic attention launch.

The three head GEMMs (forward with bias, weight gradient, K-major input gradient) are
also judged per element against tests/gemm_ref.py at N or K = out_dim in (64, 128],
as tests/test_gemm_parity_gpu.py judges the others: NaN canaries around C, NaN in the
A columns K..lda-1 of the input-gradient GEMM."""
import functools
import io

import numpy as np
import pytest
import torch

from oracle import model_ref
from tests import gemm_ref as G
from tests.test_model_widths_gpu import ffn_preactivations, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 1
SEED = 3
GATE_MARGIN = 2.0
NAN = float("nan")
F32, BF16 = torch.float32, torch.bfloat16
SHAPES = [pytest.param(256, 4, 2, 64, 68, id="256x4_T64_out68"), pytest.param(128, 2, 2, 32, 128, id="128x2_T32_out128")]
SHAPES_BF16 = SHAPES + [pytest.param(256, 4, 2, 300, 68, id="256x4_T300_out68")]


def make(D, H, amp, out, **extra):
    from neurosync_trainer_lite_amd.config import training_config
    from neurosync_trainer_lite_amd.utils.model_utils import build_model, prepare_training_components
    cfg = dict(training_config)
    cfg.update(hidden_dim=D, num_heads=H, n_layers=L, dropout=0.0, use_amp=amp, output_dim=out, **extra)
    model = build_model(cfg, DEV)
    params = model_ref.seeded_params(model_ref.param_shapes(256, D, L, out), 7)
    model.load_state_dict(params, strict=True)
    crit, opt, _ = prepare_training_components(cfg, model)
    return cfg, model, crit, opt, params


@functools.lru_cache(maxsize=None)
def data(B, T, out, seed=SEED):
    rng = np.random.default_rng(seed)
    src = torch.tensor(rng.standard_normal((B, T, 256)).astype(np.float32))
    trg = torch.tensor((rng.standard_normal((B, T, out)) * 20).astype(np.float32))
    return src, trg


@functools.lru_cache(maxsize=None)
def oracle_step(D, H, B, T, out):
    """(oracle after one step, loss, pred, gate margin) in float64, once per shape."""
    src, trg = data(B, T, out)
    params = model_ref.seeded_params(model_ref.param_shapes(256, D, L, out), 7)
    oracle = model_ref.OracleTrainer(params, H, dtype=torch.float64)
    rec = {}
    with ffn_preactivations(rec):
        o_loss, o_norm, o_pred = oracle.step(src.double(), trg.double())
    assert len(rec) == 2 * L, sorted(rec)
    margin = float("inf")
    for name, (x, pre) in rec.items():
        W, b = params[name + ".weight"].double(), params[name + ".bias"].double()
        mag = x.abs() @ W.abs().t() + b.abs()
        margin = min(margin, (pre.abs() / (2.0 ** -24 * mag)).min().item())
    return oracle, o_loss, o_pred, margin


def step(D, H, B, T, amp, out):
    from neurosync_trainer_lite_amd import _hip as K
    src, trg = data(B, T, out)
    cfg, model, crit, opt, params = make(D, H, amp, out)
    model.train()
    opt.zero_grad()
    K.kernel_counts_reset()
    pred = model(src.to(DEV))
    loss = crit(pred, trg.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().double().cpu().clone() for k, p in model.named_parameters()}
    return pred.detach().cpu(), loss.item(), grads, K.kernel_counts()


@pytest.mark.parametrize("D,H,B,T,out", SHAPES)
def test_fp32_parity_step(D, H, B, T, out):
    oracle, o_loss, o_pred, margin = oracle_step(D, H, B, T, out)
    print("fp32 D=%d out=%d batch seed %d: ReLU gate margin %.2f" % (D, out, SEED, margin))
    assert margin >= GATE_MARGIN, "the batch leaves a ReLU gate f32 cannot decide: %.2f" % margin
    cfg, model, crit, opt, params = make(D, H, False, out)
    model.eval()
    with torch.no_grad():
        infer = model(data(B, T, out)[0].to(DEV))
    assert tuple(infer.shape) == (B, T, out)
    assert rel(infer, o_pred) < 1e-4, rel(infer, o_pred)  # dropout 0: inference is the step's prediction
    pred, loss, grads, counts = step(D, H, B, T, False, out)
    print("fp32 D=%d out=%d pred rel %.3e loss %.6g / oracle %.6g" % (D, out, rel(pred, o_pred), loss, o_loss.item()))
    assert counts["loss_wide"] == 1, counts
    assert rel(pred, o_pred) < 1e-4, rel(pred, o_pred)
    assert abs(loss - o_loss.item()) < 1e-4 * abs(o_loss.item()), (loss, o_loss.item())
    for k, og in oracle.last_grads.items():
        print("%-50s out=%d fp32 %.3e" % (k, out, rel(grads[k], og)))
    worst = max((rel(grads[k], og), k) for k, og in oracle.last_grads.items())
    print("fp32 out=%d worst gradient rel" % out, worst)
    assert worst[0] < 1e-4, worst


@pytest.mark.parametrize("D,H,B,T,out", SHAPES_BF16)
def test_bf16_step(D, H, B, T, out):
    oracle, o_loss, o_pred, _ = oracle_step(D, H, B, T, out)
    y_oracle = oracle_step(D, H, B, T, 61)[0]
    y_pred, y_loss, y_grads, y_counts = step(D, H, B, T, True, 61)
    assert y_counts["loss_wide"] == 0, y_counts
    pred, loss, grads, counts = step(D, H, B, T, True, out)
    assert counts["loss_wide"] == 1, counts
    assert counts["attn_fwd_generic"] == 0 and counts["attn_bwd_generic"] == 0, counts
    print("bf16 out=%d T=%d pred rel %.3e loss %.6g / oracle %.6g" % (out, T, rel(pred, o_pred), loss, o_loss.item()))
    assert rel(pred, o_pred) < 3e-2, rel(pred, o_pred)
    assert abs(loss - o_loss.item()) < 2e-2 * abs(o_loss.item()), (loss, o_loss.item())
    for k, og in oracle.last_grads.items():
        r_new, r_61 = rel(grads[k], og), rel(y_grads[k], y_oracle.last_grads[k])
        print("%-50s out=%d %.3e out=61 %.3e" % (k, out, r_new, r_61))
        assert r_new <= max(0.1, 2 * r_61), (k, r_new, r_61)


# ---------------------------------------------------------------------------
# the head GEMMs per element, as Seq2SeqEngine.decode / backward call them
# ---------------------------------------------------------------------------
M_HEAD, D_HEAD, LD_HEAD = 256, 128, 128
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]


def rnd(*shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32) * scale).to(dtype)


def nans(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def run_head_gemm(what, A, B, M, N, Kd, ldc, **kw):
    """One nstl_gemm call into the [M][N] window of an [M + 2][ldc] NaN-filled f32 C:
    the 128 x 128 kernel ran, wrote nothing outside the window, and every element is
    within gemm_ref.bound."""
    from neurosync_trainer_lite_amd import _hip as K
    C = nans(M + 2, ldc)
    K.kernel_counts_reset()
    K.gemm(A, B, C, M, N, Kd, lda=A.stride(0), ldb=B.stride(0), ldc=ldc, **kw)
    torch.cuda.synchronize()
    c = K.kernel_counts()
    assert c["gemm128"] == 1 and c["gemm_ring"] == 0 and c["gemm4"] == 0, (what, c)
    ref, mag = G.gemm_ref(A, B, M, N, Kd, **{k: v for k, v in kw.items() if k in ("a_kmajor", "b_kmajor", "epilogue",
                                                                                   "bias", "beta")})
    live = torch.zeros_like(C, dtype=torch.bool)
    live[:M, :N] = True
    assert torch.isnan(C[~live]).all(), what + ": wrote outside the M x N window of C"
    got = C[:M, :N]
    assert not torch.isnan(got).any(), what + ": NaN in (or no write to) the window of C"
    assert (mag >= ref.abs()).all()
    ratio = ((got.double() - ref).abs() / G.bound(ref, mag, F32).clamp_min(1e-300)).max().item()
    print("%s: worst err / bound %.4f" % (what, ratio))
    assert ratio <= 1.0, "%s: worst element at %.4f of its bound" % (what, ratio)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [65, 68, 128])
def test_head_forward_gemm_with_bias(N, dtype):
    """pred [M][128] f32 = xf W^T + b with N = out_dim columns live."""
    from neurosync_trainer_lite_amd import _hip as K
    xf = rnd(M_HEAD, D_HEAD, dtype=dtype, seed=1)
    W = rnd(N, D_HEAD, dtype=dtype, scale=0.1, seed=2)
    bias = rnd(N, dtype=F32, seed=3)
    run_head_gemm("head fwd N=%d" % N, xf, W, M_HEAD, N, D_HEAD, LD_HEAD, epilogue=K.EPI_BIAS, bias=bias)


@pytest.mark.parametrize("dtype", DTYPES)
def test_head_weight_gradient_gemm(dtype):
    """grad(W) [68][D] f32 = dpred[:, :68]^T xf, dpred rows 128 wide (MN-major A, lda
    128); its columns 68..127 are the engine's zero padding, NaN here: they must not
    reach the 68 live rows of C."""
    N = 68
    dpred = nans(M_HEAD, LD_HEAD, dtype=dtype)
    dpred[:, :N] = rnd(M_HEAD, N, dtype=dtype, seed=4)
    xf = rnd(M_HEAD, D_HEAD, dtype=dtype, seed=5)
    run_head_gemm("head dW N=%d" % N, dpred, xf, N, D_HEAD, M_HEAD, D_HEAD, a_kmajor=False, b_kmajor=False, beta=0.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Kd", [65, 68, 128])
def test_head_input_gradient_gemm(Kd, dtype):
    """dres [M][D] f32 = dpred W with K = out_dim: K-major dpred with lda = 128 and NaN
    in its columns K..127 (the K tail is not read into the product), W [K][D] in place."""
    dpred = nans(M_HEAD, LD_HEAD, dtype=dtype)
    dpred[:, :Kd] = rnd(M_HEAD, Kd, dtype=dtype, seed=6)
    W = rnd(Kd, D_HEAD, dtype=dtype, scale=0.1, seed=7)
    run_head_gemm("head dX K=%d" % Kd, dpred, W, M_HEAD, D_HEAD, Kd, D_HEAD, a_kmajor=True, b_kmajor=False, beta=0.0)


# ---------------------------------------------------------------------------
# optimizer step, checkpoint, validation
# ---------------------------------------------------------------------------
def test_optimizer_step_and_state_dict_round_trip_out68():
    """One optimizer step at output_dim 68, then save / load into a fresh model: the same
    prediction bit for bit, keys and shapes those of param_shapes(..., 68)."""
    D, H, B, T, out = 256, 4, 2, 64, 68
    src, trg = data(B, T, out)
    cfg, model, crit, opt, params = make(D, H, True, out)
    model.train()
    opt.zero_grad()
    loss = crit(model(src.to(DEV)), trg.to(DEV))
    loss.backward()
    opt.step(max_norm=2.0)
    model.eval()
    with torch.no_grad():
        want = model(src.to(DEV)).cpu()
    assert tuple(want.shape) == (B, T, out)
    buf = io.BytesIO()
    torch.save(model.state_dict(), buf)
    buf.seek(0)
    state = torch.load(buf, map_location="cpu")
    shapes = model_ref.param_shapes(256, D, L, out)
    assert set(state) == set(shapes) and all(tuple(state[k].shape) == tuple(shapes[k]) for k in shapes)
    assert tuple(state["decoder.fc_output.weight"].shape) == (out, D)
    assert any(not torch.equal(state[k].cpu(), params[k].float()) for k in params), "the step changed nothing"
    cfg2, model2, _, _, _ = make(D, H, True, out)
    model2.load_state_dict(state, strict=True)
    model2.eval()
    with torch.no_grad():
        got = model2(src.to(DEV)).cpu()
    assert torch.equal(got, want)


def test_validation_keeps_the_emotion_columns_unscaled():
    """process_audio_features with a 68-output model: [num_frames, 68]; rows before the
    first blend are the model's own output of the first chunk, columns :61 divided by
    100 and 61: as they are."""
    from neurosync_trainer_lite_amd.utils.audio.processing.audio_processing import (chunk_plan, pad_audio_chunk,
                                                                                    process_audio_features)
    D, H, out, frames, size, overlap = 128, 2, 68, 300, 64, 16
    cfg, model, crit, opt, params = make(D, H, False, out, frame_size=size, overlap=overlap)
    feats = np.random.default_rng(SEED).standard_normal((frames, 256)).astype(np.float32)
    got = process_audio_features(feats, model, DEV, cfg)
    assert got.shape == (frames, out)
    chunks = [pad_audio_chunk(feats[s:e], size, 256) for s, e in chunk_plan(frames, size, overlap)]
    model.eval()
    with torch.no_grad():
        first = model.decoder(model.encoder(torch.as_tensor(np.stack(chunks)).to(DEV)))[0].cpu().numpy()
    want = first[:size - overlap].copy()
    want[:, :61] /= 100
    assert np.abs(first[:, 61:]).max() > 0
    assert np.array_equal(got[:size - overlap], want)
    assert np.array_equal(got[:size - overlap, 61:], first[:size - overlap, 61:])

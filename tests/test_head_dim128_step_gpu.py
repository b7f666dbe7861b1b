"""A whole training step and the chunked inference at head_dim 128 (D = 256, H = 2,
one layer, B = 2), against the CPU oracle in float64: a whole-tile window (T = 96) and
a ragged one (T = 100).

The bf16 step runs twice: on the generic attention kernels (NSTL_ATTN_LONG=0, the
kernels every head_dim 128 call took before the streaming kernels learned the width)
and on the default -- the engine sets NSTL_ATTN_RAGGED_OK | NSTL_ATTN_DH128_OK on every
attention call -- the streaming MFMA kernels.  The yardstick is
test_ragged_window_step_gpu's: the project's bf16 step rule (0.1 per parameter) or
twice what the generic run shows against the same float64 oracle, whichever is larger."""
import numpy as np
import pytest
import torch

from oracle import model_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, H, L, B = 256, 2, 1, 2


def make(amp):
    from neurosync_trainer_lite_amd.config import training_config
    from neurosync_trainer_lite_amd.utils.model_utils import build_model, prepare_training_components
    cfg = dict(training_config)
    cfg.update(hidden_dim=D, num_heads=H, n_layers=L, dropout=0.0, use_amp=amp)
    model = build_model(cfg, DEV)
    params = model_ref.seeded_params(model_ref.param_shapes(256, D, L, 61), 7)
    model.load_state_dict(params, strict=True)
    crit, opt, _ = prepare_training_components(cfg, model)
    return cfg, model, crit, opt, params


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def step(amp, src, trg):
    from neurosync_trainer_lite_amd import _hip as K
    cfg, model, crit, opt, params = make(amp)
    model.train()
    opt.zero_grad()
    K.kernel_counts_reset()
    pred = model(src.to(DEV))
    loss = crit(pred, trg.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().double().cpu().clone() for k, p in model.named_parameters()}
    return pred.detach().cpu(), loss.item(), grads, K.kernel_counts()


@pytest.mark.parametrize("T", [96, 100])
def test_bf16_step_head_dim128_streaming_vs_generic(T, monkeypatch):
    rng = np.random.default_rng(3)
    src = torch.tensor(rng.standard_normal((B, T, 256)).astype(np.float32))
    trg = torch.tensor((rng.standard_normal((B, T, 61)) * 20).astype(np.float32))
    params = model_ref.seeded_params(model_ref.param_shapes(256, D, L, 61), 7)
    oracle = model_ref.OracleTrainer(params, H, dtype=torch.float64)
    o_loss, o_norm, o_pred = oracle.step(src.double(), trg.double())

    monkeypatch.setenv("NSTL_ATTN_LONG", "0")
    g_pred, g_loss, g_grads, g_counts = step(True, src, trg)
    assert g_counts["attn_fwd_generic"] == 3 and g_counts["attn_bwd_generic"] == 3, g_counts
    assert g_counts["attn_fwd_long"] == 0 and g_counts["attn_bwd_long"] == 0, g_counts
    monkeypatch.delenv("NSTL_ATTN_LONG")
    pred, loss, grads, counts = step(True, src, trg)
    # one encoder self-attention, the decoder's self- and cross-attention
    assert counts["attn_fwd_long"] == 3 and counts["attn_bwd_long"] == 3, counts
    assert counts["attn_fwd_generic"] == 0 and counts["attn_bwd_generic"] == 0, counts
    print("T=%d pred rel: streaming %.3e generic %.3e; loss %.6g / %.6g / oracle %.6g"
          % (T, rel(pred, o_pred), rel(g_pred, o_pred), loss, g_loss, o_loss.item()))
    # both arms against the oracle (the generic arm checks the code around attention:
    # the bf16 GEMM RoPE epilogue at rope_dim 128 among it)
    for name, pr, ls in (("generic", g_pred, g_loss), ("streaming", pred, loss)):
        assert rel(pr, o_pred) < 3e-2, (name, rel(pr, o_pred))
        assert abs(ls - o_loss.item()) < 2e-2 * abs(o_loss.item()), (name, ls, o_loss.item())
    for k, og in oracle.last_grads.items():
        r_new, r_gen = rel(grads[k], og), rel(g_grads[k], og)
        print("%-50s streaming %.3e generic %.3e" % (k, r_new, r_gen))
        assert r_new <= max(0.1, 2 * r_gen), (k, r_new, r_gen)


def test_inference_with_300_frame_window_head_dim128():
    """process_audio_features (frame_size 300, overlap 16) on a 700-frame clip: the
    model's eval forward in bf16 with no generic attention launch, against the
    oracle forward run through the same chunk_plan / blend_chunks."""
    from neurosync_trainer_lite_amd import _hip as K
    from neurosync_trainer_lite_amd.utils.audio.processing import audio_processing as ap
    cfg, model, crit, opt, params = make(True)
    feats = np.random.default_rng(11).standard_normal((700, 256)).astype(np.float32)
    conf = dict(cfg, frame_size=300, overlap=16)
    K.kernel_counts_reset()
    got = ap.process_audio_features(feats, model, torch.device(DEV), conf)
    counts = K.kernel_counts()
    assert counts["attn_fwd_long"] >= 3 and counts["attn_fwd_generic"] == 0, counts

    class OracleSeq2Seq:
        """process_audio_features' model interface over the oracle forward"""

        def eval(self):
            return self

        def encoder(self, src):
            return src

        def decoder(self, src):
            return model_ref.seq2seq_forward(params, src.cpu(), H)

    want = ap.process_audio_features(feats, OracleSeq2Seq(), "cpu", conf)
    assert got.shape == want.shape == (700, 61)
    r = rel(torch.tensor(got), torch.tensor(want))
    print("inference rel", r)
    assert r < 3e-2, r

"""A whole training step and the chunked inference at head widths other than 64 and 128
(one layer, B = 2), against the CPU oracle in float64: (hidden_dim, heads, window) =
(128, 16, 64), (256, 8, 100), (384, 8, 64), (384, 4, 300), i.e. head_dim 8, 32, 48 and
96, two of the windows ragged.

The bf16 step runs twice: on the generic attention kernels (NSTL_ATTN_LONG=0, the
kernels every such call took before the streaming kernels learned the widths) and on
the default -- the engine sets NSTL_ATTN_RAGGED_OK | NSTL_ATTN_DH128_OK |
NSTL_ATTN_DHANY_OK on every attention call -- the streaming MFMA kernels.  The yardstick
is tests/test_head_dim128_step_gpu.py's: each arm against the float64 oracle, the
streaming arm held to the project's bf16 step rule (0.1 per parameter) or twice what the
generic run shows against the same oracle, whichever is larger -- never to itself."""
import numpy as np
import pytest
import torch

from oracle import model_ref
from tests import attn_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, B = 1, 2


def make(D, H, amp, dropout=0.0):
    from neurosync_trainer_lite_amd.config import training_config
    from neurosync_trainer_lite_amd.utils.model_utils import build_model, prepare_training_components
    cfg = dict(training_config)
    cfg.update(hidden_dim=D, num_heads=H, n_layers=L, dropout=dropout, use_amp=amp)
    model = build_model(cfg, DEV)
    params = model_ref.seeded_params(model_ref.param_shapes(256, D, L, 61), 7)
    model.load_state_dict(params, strict=True)
    crit, opt, _ = prepare_training_components(cfg, model)
    return cfg, model, crit, opt, params


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def batch(T, seed=3):
    rng = np.random.default_rng(seed)
    src = torch.tensor(rng.standard_normal((B, T, 256)).astype(np.float32))
    trg = torch.tensor((rng.standard_normal((B, T, 61)) * 20).astype(np.float32))
    return src, trg


def step(D, H, src, trg, dropout=0.0):
    from neurosync_trainer_lite_amd import _hip as K
    cfg, model, crit, opt, params = make(D, H, True, dropout)
    model.train()
    opt.zero_grad()
    K.kernel_counts_reset()
    pred = model(src.to(DEV))
    loss = crit(pred, trg.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().double().cpu().clone() for k, p in model.named_parameters()}
    return pred.detach().cpu(), loss.item(), grads, K.kernel_counts(), model


@pytest.mark.parametrize("D,H,T", [(128, 16, 64), (256, 8, 100), (384, 8, 64), (384, 4, 300)])
def test_bf16_step_streaming_vs_generic(D, H, T, monkeypatch):
    src, trg = batch(T)
    params = model_ref.seeded_params(model_ref.param_shapes(256, D, L, 61), 7)
    oracle = model_ref.OracleTrainer(params, H, dtype=torch.float64)
    o_loss, o_norm, o_pred = oracle.step(src.double(), trg.double())

    monkeypatch.setenv("NSTL_ATTN_LONG", "0")
    g_pred, g_loss, g_grads, g_counts, _ = step(D, H, src, trg)
    assert g_counts["attn_fwd_generic"] == 3 and g_counts["attn_bwd_generic"] == 3, g_counts
    assert g_counts["attn_fwd_long"] == 0 and g_counts["attn_bwd_long"] == 0, g_counts
    monkeypatch.delenv("NSTL_ATTN_LONG")
    pred, loss, grads, counts, _ = step(D, H, src, trg)
    # one encoder self-attention, the decoder's self- and cross-attention
    assert counts["attn_fwd_long"] == 3 and counts["attn_bwd_long"] == 3, counts
    assert counts["attn_fwd_generic"] == 0 and counts["attn_bwd_generic"] == 0, counts
    print("D=%d H=%d T=%d pred rel: streaming %.3e generic %.3e; loss %.6g / %.6g / oracle %.6g"
          % (D, H, T, rel(pred, o_pred), rel(g_pred, o_pred), loss, g_loss, o_loss.item()))
    # both arms against the oracle (the generic arm checks the code around attention)
    for name, pr, ls in (("generic", g_pred, g_loss), ("streaming", pred, loss)):
        assert rel(pr, o_pred) < 3e-2, (name, rel(pr, o_pred))
        assert abs(ls - o_loss.item()) < 2e-2 * abs(o_loss.item()), (name, ls, o_loss.item())
    for k, og in oracle.last_grads.items():
        r_new, r_gen = rel(grads[k], og), rel(g_grads[k], og)
        print("%-50s streaming %.3e generic %.3e" % (k, r_new, r_gen))
        assert r_new <= max(0.1, 2 * r_gen), (k, r_new, r_gen)


def test_dropout_step_stores_the_hash_stream_keep_words():
    """One dropout-0.3 step at head_dim 32 (D = 256, H = 8, T = 64): it runs on the
    streaming kernels, the loss is finite, and layer 0's stored keep words of the three
    attention sites are attn_ref.keep_words of that site's seed, bit for bit."""
    from neurosync_trainer_lite_amd.engine import _seed
    D, H, T, p = 256, 8, 64, 0.3
    src, trg = batch(T)
    torch.manual_seed(7)
    pred, loss, grads, counts, model = step(D, H, src, trg, dropout=p)
    assert counts["attn_fwd_long"] == 3 and counts["attn_bwd_long"] == 3, counts
    assert counts["attn_fwd_generic"] == 0 and counts["attn_bwd_generic"] == 0, counts
    assert np.isfinite(loss) and torch.isfinite(pred).all()
    assert all(torch.isfinite(g).all() for g in grads.values())
    eng = model.engine(torch.device(DEV))
    bb, base = eng.saved["bb"], eng.saved["seed"]
    assert eng.saved["p"] == p and base != 0
    nt = (T + 15) // 16
    nw = B * H * nt * nt * 4
    for enc, buf, site in ((True, bb.e_mask, "attn"), (False, bb.d_mask, "attn"), (False, bb.d_maskc, "xattn")):
        got = buf[0][:nw].cpu().numpy().view(np.uint64)
        want = A.keep_words(A.keep(_seed(base, enc, 0, site), B * H, T, p), T)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s %s: %d of %d keep words differ" % ("encoder" if enc else "decoder", site, bad.size, nw)


def test_inference_with_300_frame_window_head_dim32():
    """process_audio_features (frame_size 300, overlap 16) on a 700-frame clip at
    D = 256, H = 8: the model's eval forward in bf16 with no generic attention launch,
    against the oracle forward run through the same chunk_plan / blend_chunks."""
    from neurosync_trainer_lite_amd import _hip as K
    from neurosync_trainer_lite_amd.utils.audio.processing import audio_processing as ap
    D, H = 256, 8
    cfg, model, crit, opt, params = make(D, H, True)
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

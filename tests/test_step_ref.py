"""CPU proof of the mask-injecting oracle (oracle/model_ref.py `masks`) and of the
mask provider (tests/step_ref.py) that tests/test_dropout_step_parity_gpu.py judges a
whole dropout-on training step by.  No GPU.

A 2-layer model (D 64, H 2, B 2, T 16, seeded_params) in float64:
  * all-ones masks reproduce the dropout-free oracle;
  * each of the 13 per-layer sites (5 encoder, 8 decoder; engine._SITE has nine names,
    `drop2` is the encoder's and `drop3` the decoder's FFN branch) of each layer is
    consumed;
  * six deliberately wrong references (the mistakes an engine could make between
    kernels) each move some gradient tensor by more than MUTANT_FLOOR, the largest
    value any gate of the GPU test can take (its bf16 gates are capped at 0.1, its fp32
    gate is 1e-4).  The table is printed (profiles/dropout_step_parity_errors.txt)."""
import types

import numpy as np
import pytest
import torch

from neurosync_trainer_lite_amd.engine import Seq2SeqEngine, _seed
from oracle import model_ref
from tests import step_ref as S

D, H, L, B, T, P = 64, 2, 2, 2, 16, 0.3
BASE = 0x1234_5678_9ABC_DEF0 % (1 << 62)
# every gate of tests/test_dropout_step_parity_gpu.py is at or below this (BF16_GRAD_CAP)
MUTANT_FLOOR = 0.1


def rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


@pytest.fixture(scope="module", autouse=True)
def one_thread():
    """These tensors are tiny: a thread pool only costs (20 ms a step on one thread)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def problem():
    params = model_ref.seeded_params(model_ref.param_shapes(256, D, L, 61), 17)
    rng = np.random.default_rng(18)
    src = torch.tensor(rng.standard_normal((B, T, 256)))
    trg = torch.tensor(rng.standard_normal((B, T, 61)) * 20)
    masks = S.site_masks(BASE, B, T, D, H, L, P)
    return params, src, trg, masks


def run(problem, masks, dropout=P):
    params, src, trg, _ = problem
    o = model_ref.OracleTrainer(params, H, dropout=dropout, dtype=torch.float64)
    loss, norm, pred = o.step(src, trg, masks=masks)
    return loss.item(), pred, o.last_grads


@pytest.fixture(scope="module")
def right(problem):
    return run(problem, problem[3])


def test_site_keys_and_shapes(problem):
    masks = problem[3]
    assert len(masks) == L * (len(S.ENC_SITES) + len(S.DEC_SITES)) == L * 13
    for (enc, l, s), m in masks.items():
        want = (B, H, T, T) if s in ("attn", "xattn") else (B, T, 4 * D) if s == "ffn" else (B, T, D)
        assert tuple(m.shape) == want and m.dtype == torch.float64, (enc, l, s)
        vals = set(m.unique().tolist())
        assert vals == {0.0, S.site_scale(s, P)}, (enc, l, s, vals)


def test_all_ones_masks_equal_dropout_free_oracle(problem):
    ones = {k: torch.ones_like(m) for k, m in problem[3].items()}
    loss1, pred1, g1 = run(problem, ones)
    loss0, pred0, g0 = run(problem, None, dropout=0.0)
    assert abs(loss1 - loss0) <= 1e-12 * abs(loss0)
    assert rel(pred1, pred0) <= 1e-12
    for k in g0:
        assert rel(g1[k], g0[k]) <= 1e-12, k


def test_masks_none_keeps_torch_rng_stream(problem):
    """masks=None is F.dropout as before: the same draws in the same order (the layer
    bodies below restate the functions as they stood before `masks`)."""
    import torch.nn.functional as F
    params, src, _, _ = problem
    p64 = {k: v.double() for k, v in params.items()}
    M = model_ref

    def enc_layer(p, name, x):
        d = lambda t: F.dropout(t, P, True)
        a = d(M.attention(p, name + ".self_attn", x, x, H, P, True))
        x = M.layer_norm(p, name + ".norm1", x + d(a))
        f = M.ffn(p, name + ".ffn", x, P, True)
        return M.layer_norm(p, name + ".norm2", x + d(f))

    def dec_layer(p, name, x, mem):
        d = lambda t: F.dropout(t, P, True)
        a = d(M.attention(p, name + ".self_attn", x, x, H, P, True))
        x = M.layer_norm(p, name + ".norm1", x + d(a))
        c = d(M.attention(p, name + ".multihead_attn", x, mem, H, P, True))
        x = M.layer_norm(p, name + ".norm2", x + d(c))
        f = M.ffn(p, name + ".ffn", x, P, True)
        return M.layer_norm(p, name + ".norm3", x + d(f))

    torch.manual_seed(5)
    x = M.global_pe(M.linear(p64, "encoder.embedding", src))
    for i in range(L):
        x = enc_layer(p64, "encoder.transformer_encoder.%d" % i, x)
    mem = M.layer_norm(p64, "encoder.layer_norm", x)
    x = M.global_pe(mem)
    for i in range(L):
        x = dec_layer(p64, "decoder.transformer_decoder.%d" % i, x, mem)
    want = M.linear(p64, "decoder.fc_output", M.layer_norm(p64, "decoder.layer_norm", x))
    torch.manual_seed(5)
    got = M.seq2seq_forward(p64, src, H, P, True)
    assert torch.equal(got, want)
    # and eval draws nothing
    state = torch.get_rng_state()
    M.seq2seq_forward(p64, src, H, P, False)
    assert torch.equal(state, torch.get_rng_state())


@pytest.mark.parametrize("layer", [0, 1])
def test_every_site_is_consumed(problem, right, layer):
    masks = problem[3]
    params, src, trg, _ = problem
    p64 = {k: v.double() for k, v in params.items()}
    for key in [k for k in S.site_keys(L) if k[1] == layer]:
        m = dict(masks)
        m[key] = torch.ones_like(masks[key])
        with torch.no_grad():
            loss = model_ref.loss_fn(model_ref.seq2seq_forward(p64, src, H, P, True, m), trg).item()
        assert abs(loss - right[0]) > 1e-9 * abs(right[0]), key


# ---------------------------------------------------------------------------- mutants
def _each_layer(fn):
    def build(masks):
        m = dict(masks)
        for enc in (True, False):
            for l in range(L):
                fn(m, enc, l)
        return m
    return build


def _drop1_takes_drop2_seed(m, enc, l):
    m[(enc, l, "drop1")] = (S.site_keep(_seed(BASE, enc, l, "drop2"), "drop1", B, T, D, H, P).double()
                            * S.site_scale("drop1", P))


def _resid_unscaled(m, enc, l):
    m[(enc, l, "resid")] = m[(enc, l, "resid")] * (1.0 - P)


def _attn_transposed(m, enc, l):
    m[(enc, l, "attn")] = m[(enc, l, "attn")].transpose(-1, -2)


def _xattn_takes_attn_seed(m, enc, l):
    if not enc:
        m[(enc, l, "xattn")] = m[(enc, l, "attn")]


def _layer1_reuses_layer0(masks):
    return {(enc, l, s): masks[(enc, 0, s)] for enc, l, s in masks}


def _ffn_mask_before_bias(p, name, x, dropout=0.0, training=False, masks=None, where=None):
    """wrong on purpose: relu((x W^T) mask + b) in place of relu(x W^T + b) mask"""
    z = torch.nn.functional.linear(x, p[name + ".linear1.weight"]) * masks[where]
    return model_ref.linear(p, name + ".linear2", torch.relu(z + p[name + ".linear1.bias"]))


MUTANTS = [
    ("drop1 takes drop2's seed", _each_layer(_drop1_takes_drop2_seed), None),
    ("layer 1 reuses layer 0's masks", _layer1_reuses_layer0, None),
    ("resid mask without its 1/(1-p)", _each_layer(_resid_unscaled), None),
    ("attn mask transposed (query <-> key)", _each_layer(_attn_transposed), None),
    ("ffn mask before the bias add", dict, _ffn_mask_before_bias),
    ("xattn takes attn's seed", _each_layer(_xattn_takes_attn_seed), None),
]


def test_mutants_clear_every_gate(problem, right, monkeypatch):
    rows = []
    for name, build, wrong_ffn in MUTANTS:
        with monkeypatch.context() as mp:
            if wrong_ffn is not None:
                mp.setattr(model_ref, "ffn", wrong_ffn)
            loss, pred, grads = run(problem, build(problem[3]))
        dev = {k: rel(grads[k], right[2][k]) for k in grads}
        worst = max(dev, key=dev.get)
        rows.append((name, worst, dev[worst], "%d/%d" % (sum(d > MUTANT_FLOOR for d in dev.values()), len(dev)),
                     abs(loss - right[0]) / abs(right[0]), rel(pred, right[1])))
    print("\nmutant table (D %d H %d L %d B %d T %d p %.1f, float64; deviation from the right reference)" %
          (D, H, L, B, T, P))
    print("%-38s %-60s %10s %8s %10s %10s" % ("mutant", "gradient that moves most", "grad rel", "> 0.1", "loss rel",
                                              "pred rel"))
    for r in rows:
        print("%-38s %-60s %10.3e %8s %10.3e %10.3e" % r)
    for name, worst, d, _, _, _ in rows:
        assert d > MUTANT_FLOOR, (name, worst, d)


# ------------------------------------------------------------------------ sanity
def test_mask_means_are_one(problem):
    for key, m in problem[3].items():
        n = m.numel()
        sigma = (P * (1 - P) / n) ** 0.5 / (1 - P)
        assert abs(m.mean().item() - 1.0) < 5 * sigma, (key, m.mean().item(), sigma)


def test_seed_salt_changes_every_mask():
    eng = types.SimpleNamespace(p=P, seed_salt=0)
    seeds = []
    for salt in (0, 1):
        eng.seed_salt = salt
        torch.manual_seed(9)
        seeds.append(Seq2SeqEngine.draw_seed(eng))
    torch.manual_seed(9)
    draw = int(torch.randint(0, 2 ** 62, (1,)).item())
    assert seeds == [S.salted_seed(draw, 0), S.salted_seed(draw, 1)] and seeds[0] != seeds[1]
    m0, m1 = (S.site_masks(s, B, T, D, H, L, P) for s in seeds)
    for key in m0:
        assert not torch.equal(m0[key], m1[key]), key

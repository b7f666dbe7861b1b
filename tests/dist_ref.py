"""TEST INFRA: a scripted multi-rank epoch and the float64 reference that judges it, with
no GPU dependency.  Built on tests/epoch_ref.py (gates, schedule, the Adam bound),
tests/step_ref.py (the masks of a seed) and oracle/model_ref.py.  tests/test_dist_ref.py
proves what is here on the CPU and shows seven mistakes of the kind looked for breaking the
gates; tests/test_dist_epoch_gpu.py drives training_utils.train_one_epoch_multi_gpu through
the scripts on one card and judges every event by it.  Never imported by the package.

The script.  An epoch is a plain list of (src, trg) CPU tensors, as in epoch_ref:

  BF16  D256 H4 L2 p 0.1, bf16   batches B4 T64: 256 rows, so a decoder layer's weight
        gradients leave in one grouped, deferred launch (engine._defer / _dw_flush): the
        flush is what reducer.ready must follow.
  FP32  D128 H2 L2 p 0.1, f32    batches B2 T32.

3 x world + 1 training batches (rank r of step s takes batch s x world + r; the last one is
the leftover rank_batches must drop), two validation batches, validation every 2 steps (rank
0 alone, after steps 0 and 2 of each epoch), two epochs with epoch_ref's schedule (lr halves
in epoch 1).  World sizes 2 and 3: three is no power of two, gives every owner two receive
slots, and engine.ARENA_ALIGN = 64 x 840 splits into three shards.

The reference.  teacher_forced_dp_step is one float64 oracle step from a given state whose
gradient is the sum over the ranks of the gradient of loss_r / world, each rank's masks those
of its salted seed (epoch_ref.epoch_seeds(..., seed_salt=r)); clip and Adam as
epoch_ref.teacher_forced_step; the loss returned is the mean of the ranks' losses.

The arena.  layout() restates the engine's gradient arena (engine._arena_order, _pad64 and
ARENA_ALIGN are the engine's own; the GPU test asserts the offsets equal the engine's): the
matrices in reverse backward order, padded to n_shardable, then the f32 vectors; and the
prefix that is final at each reducer.ready call site of engine.backward (ready_sites).  The
small bucket of a run is chosen from it (small_bucket)."""
import types

import numpy as np
import torch

from neurosync_trainer_lite_amd import engine as _engine
from oracle import model_ref
from tests import epoch_ref as E
from tests import step_ref as S

IN_DIM, OUT_DIM = E.IN_DIM, E.OUT_DIM
PARAM_SEED = 43
DATA_SEED = 500
EPOCH_SEED = E.EPOCH_SEED
CLIP = E.CLIP
WORLDS = (2, 3)
STEPS = 3      # per rank and epoch
EPOCHS = 2
INTERVAL = 2   # validation_interval

SCRIPTS = {
    "BF16": dict(D=256, H=4, L=2, p=0.1, amp=True, B=4, T=64),
    "FP32": dict(D=128, H=2, L=2, p=0.1, amp=False, B=2, T=32),
}
GATES = {"BF16": E.BF16_GATES, "FP32": E.FP32_GATES}


def config(name):
    sc = SCRIPTS[name]
    cfg = dict(E.training_config)
    cfg.update(hidden_dim=sc["D"], num_heads=sc["H"], n_layers=sc["L"], dropout=sc["p"], use_amp=sc["amp"],
               warmup_epochs=0, n_epochs=EPOCHS, checkpoint_path="out/checkpoints/checkpoint.pth")
    return cfg


def shapes(name):
    sc = SCRIPTS[name]
    return model_ref.param_shapes(IN_DIM, sc["D"], sc["L"], OUT_DIM)


def params(name):
    return model_ref.seeded_params(shapes(name), PARAM_SEED)


def batches(name, world):
    """(training list of 3 x world + 1 batches, validation list of 2)."""
    sc = SCRIPTS[name]
    rng = np.random.default_rng(DATA_SEED + world)

    def one():
        src = torch.tensor(rng.standard_normal((sc["B"], sc["T"], IN_DIM)).astype(np.float32))
        trg = torch.tensor((rng.standard_normal((sc["B"], sc["T"], OUT_DIM)) * 20).astype(np.float32))
        return src, trg
    return [one() for _ in range(STEPS * world + 1)], [one() for _ in range(2)]


def events():
    """One epoch as train_one_epoch_multi_gpu runs it: [("train", s) | ("val", j)]; step s
    is batch s x world + r on rank r; a validation forward (rank 0 only) after step s when
    s % INTERVAL == 0, the validation list read from its start in every epoch."""
    out, j = [], 0
    for s in range(STEPS):
        out.append(("train", s))
        if s % INTERVAL == 0:
            out.append(("val", j % 2))
            j += 1
    return out


def rank_seeds(epoch, rank):
    """Base seeds of rank `rank`'s STEPS training forwards of `epoch` (every rank draws
    the same torch numbers; the engine salts them with the rank)."""
    return E.epoch_seeds(epoch, STEPS, seed_salt=rank)


def masks_of(name, seed):
    sc = SCRIPTS[name]
    return S.site_masks(seed, sc["B"], sc["T"], sc["D"], sc["H"], sc["L"], sc["p"])


def rank_inputs(name, world, epoch, s, seed_salts=None):
    """[(src, trg, masks)] of step s of `epoch`, one per rank.  seed_salts: the salt of each
    rank (default: its rank)."""
    train, _ = batches(name, world)
    out = []
    for r in range(world):
        salt = r if seed_salts is None else seed_salts[r]
        src, trg = train[s * world + r]
        out.append((src, trg, masks_of(name, rank_seeds(epoch, salt)[s])))
    return out


# ------------------------------------------------------------------------ the reference
def teacher_forced_dp_step(params, m, v, step, lr, ranks, num_heads, wd, clip=CLIP):
    """One float64 data-parallel oracle step from a given state.  ranks: [(src, trg, masks)],
    one per rank.  The gradient is sum_r grad(loss_r / world), added in rank order; clip and
    Adam follow as in epoch_ref.teacher_forced_step.  Nothing of the caller's is modified."""
    world = len(ranks)
    keys = list(params.keys())
    p = {k: params[k].detach().to("cpu", torch.float64).clone().requires_grad_(True) for k in keys}
    leaves = [p[k] for k in keys]
    losses, preds, rank_grads = [], [], []
    for src, trg, masks in ranks:
        pred = model_ref.seq2seq_forward(p, src.double(), num_heads, 0.0, masks is not None, masks)
        loss = model_ref.loss_fn(pred, trg.double())
        rank_grads.append(torch.autograd.grad(loss / world, leaves))
        losses.append(loss.item())
        preds.append(pred.detach())
    grads = [g.clone() for g in rank_grads[0]]
    for gr in rank_grads[1:]:
        for g, x in zip(grads, gr):
            g.add_(x)
    last = {k: g.clone() for k, g in zip(keys, grads)}
    mm = [m[k].detach().to("cpu", torch.float64).clone() for k in keys]
    vv = [v[k].detach().to("cpu", torch.float64).clone() for k in keys]
    with torch.no_grad():
        total = model_ref.clip_grad_norm(grads, clip)
        model_ref.adam_l2_step(leaves, grads, mm, vv, int(step) + 1, lr, weight_decay=wd)
    return dict(loss=sum(losses) / world if world > 1 else losses[0], losses=losses, preds=preds,
                pred=torch.cat(preds), norm=total.item(), grads=last,
                rank_grads=[dict(zip(keys, g)) for g in rank_grads], params={k: p[k].detach() for k in keys},
                m=dict(zip(keys, mm)), v=dict(zip(keys, vv)), step=int(step) + 1)


# ---------------------------------------------------------------------------- the arena
def layout(name):
    """The engine's arena of the script's model, restated from its shapes:
    offsets {key: (offset, numel, shape)}, n_shardable, numel, end_of {key: final prefix}."""
    sc, shp = SCRIPTS[name], shapes(name)
    order = _engine.Seq2SeqEngine._arena_order(types.SimpleNamespace(L=sc["L"]))
    assert sorted(order) == sorted(shp)
    mats = [n for n in order if len(shp[n]) > 1]
    vecs = [n for n in order if len(shp[n]) <= 1]
    offsets, off = {}, 0
    for n in mats:
        k = int(np.prod(shp[n]))
        offsets[n] = (off, k, tuple(shp[n]))
        off += _engine._pad64(k)
    n_shardable = off = (off + _engine.ARENA_ALIGN - 1) // _engine.ARENA_ALIGN * _engine.ARENA_ALIGN
    for n in vecs:
        k = int(np.prod(shp[n]))
        offsets[n] = (off, k, tuple(shp[n]))
        off += _engine._pad64(k)
    end_of, hi = {}, 0
    for n in order:
        o, k, _ = offsets[n]
        if len(shp[n]) > 1:
            hi = o + _engine._pad64(k)
        end_of[n] = hi
    return types.SimpleNamespace(order=order, offsets=offsets, n_shardable=n_shardable, numel=off, end_of=end_of,
                                 L=sc["L"])


def ready_sites(lay, enc_grouped=True):
    """(parameter name, final prefix) at each reducer.ready call site of engine.backward, in
    call order.  enc_grouped (the engine's default): the encoder's weight gradients leave in
    one grouped launch per ENC_GROUP layers, and ready follows that launch only."""
    names = ["decoder.layer_norm.bias"]
    names += ["decoder.transformer_decoder.%d.self_attn.v_linear.bias" % l for l in reversed(range(lay.L))]
    names.append("encoder.layer_norm.bias")
    names += ["encoder.transformer_encoder.%d.self_attn.v_linear.bias" % l for l in reversed(range(lay.L))
              if not enc_grouped or l % _engine.ENC_GROUP == 0]
    return [(n, lay.end_of[n]) for n in names]


def min_growth(lay):
    """The smallest growth of the final prefix between two consecutive ready call sites."""
    ends = [0] + [e for _, e in ready_sites(lay, enc_grouped=False)]
    return min(b - a for a, b in zip(ends, ends[1:]) if b > a)


def smallest_layer(lay):
    """Elements of the smallest transformer layer's matrices (an encoder layer)."""
    return sum(_engine._pad64(k) for n, (o, k, shp) in lay.offsets.items()
               if n.startswith("encoder.transformer_encoder.0.") and len(shp) > 1)


def small_bucket(lay):
    """Bucket (elements) of the small-bucket runs: below min_growth, so every ready call
    that extends the prefix releases at least one bucket; the largest multiple of 1000 that
    divides the shard of no world size, so bucket edges do not line up with shard or tensor
    boundaries: they fall inside layers, inside the k|v block and across shard boundaries."""
    b = (min_growth(lay) - 1) // 1000 * 1000
    while b > 0 and any((lay.n_shardable // w) % b == 0 for w in WORLDS):
        b -= 1000
    assert 0 < b < min_growth(lay)
    return b


def flat(lay, tensors, dtype=None):
    """{key: tensor} as one flat arena (padding zero)."""
    any_t = next(iter(tensors.values()))
    out = torch.zeros(lay.numel, dtype=dtype or any_t.dtype)
    for n, (o, k, shp) in lay.offsets.items():
        out[o:o + k] = tensors[n].detach().reshape(-1).to(out.dtype)
    return out


def unflat(lay, arena):
    return {n: arena[o:o + k].view(shp) for n, (o, k, shp) in lay.offsets.items()}

"""CPU proof of tests/dist_ref.py, which tests/test_dist_epoch_gpu.py judges a scripted
multi-rank epoch by.  No GPU.

  * teacher_forced_dp_step at world 1 is epoch_ref.teacher_forced_step exactly, and its
    gradient is the autograd gradient of sum_r loss_r / world.
  * layout() has the properties the small bucket is chosen for.
  * Mutants.  An f32 CPU stand-in of the sharded step on the flat arena (per-rank f32
    backward of loss_r / world through model_ref, the owner's sum own + slots in rank order,
    the all-reduced vector tail, the clip norm from every shard's partials, Adam, one weight
    replica per rank as the all-gather leaves it) runs the FP32 script's first epoch at
    world 3, with one switch per mistake.  Every step is judged as the GPU test judges a run:
      oracle gates   teacher_forced_dp_step from the run's own state before the step, the
                     ranks' salted seeds: grad, pred, loss, norm, param, param_mean
                     (epoch_ref.broken_gates with FP32_GATES; pred over every rank's rows)
      exact gates    replicas: every rank's weights after the step are bit-identical
                     (gate 3 of the GPU test); equal: the run equals the clean run bit for
                     bit (gates 1 and 2: small bucket against default, push against zero1)
    The clean run breaks none at worlds 2 and 3 over both epochs.  Each mutant breaks at
    least one gate at the step named; the table printed says which, and which mutants only
    the exact gates separate."""
import pytest
import torch

from oracle import model_ref
from tests import dist_ref as R
from tests import epoch_ref as E

NAME = "FP32"
SC = R.SCRIPTS[NAME]
CFG = R.config(NAME)
LAY = R.layout(NAME)


@pytest.fixture(scope="module", autouse=True)
def few_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(4, n))
    yield
    torch.set_num_threads(n)


# ------------------------------------------------------------------------ the reference
def test_world_one_is_the_single_process_step():
    (src, trg), = R.batches(NAME, 1)[0][:1]
    masks = R.masks_of(NAME, R.rank_seeds(0, 0)[0])
    p = R.params(NAME)
    m = {k: torch.randn(v.shape, generator=torch.Generator().manual_seed(1)) * 1e-3 for k, v in p.items()}
    v = {k: torch.rand(q.shape, generator=torch.Generator().manual_seed(2)) * 1e-6 for k, q in p.items()}
    a = E.teacher_forced_step(p, m, v, 3, 2.5e-5, src, trg, masks, SC["H"], CFG["weight_decay"])
    b = R.teacher_forced_dp_step(p, m, v, 3, 2.5e-5, [(src, trg, masks)], SC["H"], CFG["weight_decay"])
    assert a["loss"] == b["loss"] and a["norm"] == b["norm"] and a["step"] == b["step"] == 4
    assert torch.equal(a["pred"], b["pred"])
    for k in p:
        for key in ("grads", "params", "m", "v"):
            assert torch.equal(a[key][k], b[key][k]), (key, k)


@pytest.mark.parametrize("world", R.WORLDS)
def test_gradient_is_that_of_the_summed_scaled_losses(world):
    ranks = R.rank_inputs(NAME, world, 0, 1)
    p = R.params(NAME)
    zeros = {k: torch.zeros_like(q) for k, q in p.items()}
    ref = R.teacher_forced_dp_step(p, zeros, zeros, 0, 1e-4, ranks, SC["H"], CFG["weight_decay"])
    leaves = {k: q.double().clone().requires_grad_(True) for k, q in p.items()}
    total = sum(model_ref.loss_fn(model_ref.seq2seq_forward(leaves, s.double(), SC["H"], 0.0, True, mk), t.double())
                / world for s, t, mk in ranks)
    total.backward()
    for k in p:
        assert E.rel(ref["grads"][k], leaves[k].grad) < 1e-12, k
    assert ref["loss"] == pytest.approx(total.item(), rel=1e-14)
    # the ranks see different masks and different batches
    assert not torch.equal(ranks[0][2][(True, 0, "resid")], ranks[1][2][(True, 0, "resid")])
    assert len({r for w in range(3) for r in R.rank_seeds(0, w)}) == 3 * R.STEPS


def test_script_and_layout():
    assert R.events() == [("train", 0), ("val", 0), ("train", 1), ("train", 2), ("val", 1)]
    for name in R.SCRIPTS:
        lay = R.layout(name)
        cfg = R.config(name)
        assert E.lr_at(cfg, 1) == 0.5 * E.lr_at(cfg, 0)
        for w in R.WORLDS:
            train, val = R.batches(name, w)
            assert len(train) == R.STEPS * w + 1 and len(train) // w == R.STEPS and len(val) == 2
            assert lay.n_shardable % (w * 64) == 0
        b = R.small_bucket(lay)
        sites = R.ready_sites(lay)
        ends = [0] + [e for _, e in sites]
        assert all(y - x > b for x, y in zip(ends, ends[1:])), (b, ends)
        assert lay.n_shardable - ends[-1] + b < R.smallest_layer(lay)  # what finish() is left with
        # the k|v block lies behind the decoder layers and in front of the encoder's prefix
        kv = lay.offsets["decoder.transformer_decoder.0.multihead_attn.k_linear.weight"][0]
        assert sites[lay.L][1] <= kv < sites[lay.L + 1][1]
        # bucket edges inside the k|v block, and a bucket across each shard boundary
        assert any(kv < e * b < sites[lay.L + 1][1] for e in range(1, lay.n_shardable // b))
        for w in R.WORLDS:
            assert all((r * (lay.n_shardable // w)) % b for r in range(1, w))
        print("%s: arena %d + %d, ready at %s, bucket %d" % (name, lay.n_shardable, lay.numel - lay.n_shardable,
                                                            ends[1:], b))


# ------------------------------------------------------------------------------ mutants
class StandIn:
    """The sharded data-parallel step in f32 on flat arenas (no switch: the clean step)."""

    def __init__(self, world, mutant=None, at=2):
        self.world, self.mutant, self.at = world, mutant, at
        self.shard = LAY.n_shardable // world
        self.p = R.flat(LAY, R.params(NAME), torch.float32)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.replicas = [self.p.clone() for _ in range(world)]
        self.prev = [torch.zeros_like(self.p) for _ in range(world)]  # each rank's gradient arena as the last backward left it
        self.t = 0

    def step(self, epoch, s, lr, n):
        """n: 1-based index of the step in the run."""
        w, hit = self.world, self.mutant is not None and n == self.at
        salts = [0] * w if hit and self.mutant == "same_salt" else None
        ranks = R.rank_inputs(NAME, w, epoch, s, seed_salts=salts)
        arenas, losses, preds = [], [], []
        for r, (src, trg, masks) in enumerate(ranks):
            leaves = {k: x.clone().requires_grad_(True) for k, x in R.unflat(LAY, self.replicas[r]).items()}
            pred = model_ref.seq2seq_forward(leaves, src, SC["H"], 0.0, True, {k: x.float() for k, x in masks.items()})
            loss = model_ref.loss_fn(pred, trg)
            scale = 1.0 if hit and self.mutant == "no_scale" else 1.0 / w
            keys = list(leaves)
            g = torch.autograd.grad(loss * scale, [leaves[k] for k in keys])
            arenas.append(R.flat(LAY, dict(zip(keys, g))))
            losses.append(loss.item())
            preds.append(pred.detach())
        fresh = [a.clone() for a in arenas]
        ns, sh = LAY.n_shardable, self.shard
        if hit and self.mutant == "stale_bucket":
            # rank 1's bucket inside decoder layer 1's FFN left before its last writer ran
            b = R.small_bucket(LAY)
            lo = LAY.offsets["decoder.transformer_decoder.1.ffn.linear1.weight"][0] // b * b + b
            arenas[1][lo:lo + b] = self.prev[1][lo:lo + b]
        g = torch.zeros_like(self.p)
        for o in range(w):  # owner o: own slice + the slots in rank order
            senders = [r for r in range(w) if r != o]
            if hit and self.mutant == "slot_collision" and o == 0:
                senders = senders[1:]  # ranks 1 and 2 wrote the same slot: rank 1's slice is gone
            acc = arenas[o][o * sh:(o + 1) * sh].clone()
            for r in senders:
                acc += arenas[r][o * sh:(o + 1) * sh]
            g[o * sh:(o + 1) * sh] = acc
        if hit and self.mutant == "tail_unreduced":
            g[ns:] = arenas[0][ns:]
        else:
            g[ns:] = sum(a[ns:] for a in arenas)
        parts = [g[o * sh:(o + 1) * sh].double().pow(2).sum() for o in range(w)] + [g[ns:].double().pow(2).sum()]
        if hit and self.mutant == "norm_one_shard":
            parts = [parts[0], parts[-1]]
        total = torch.stack(parts).sum().sqrt().float()
        self.grads = R.unflat(LAY, g.clone())
        self.before = dict(p=R.unflat(LAY, self.p.clone()), m=R.unflat(LAY, self.m.clone()), v=R.unflat(LAY, self.v.clone()))
        old = self.p.clone()
        g.mul_(torch.clamp(CLIP_T / (total + 1e-6), max=1.0))
        self.t += 1
        model_ref.adam_l2_step([self.p], [g], [self.m], [self.v], self.t, lr, weight_decay=CFG["weight_decay"])
        self.replicas = [self.p.clone() for _ in range(w)]
        if hit and self.mutant == "stale_peer_shard":
            self.replicas[1][:sh] = old[:sh]  # rank 0's updated shard never reached rank 1
        self.prev = fresh
        return dict(loss=sum(losses) / w, norm=total.item(), pred=torch.cat(preds), grads=self.grads,
                    params=R.unflat(LAY, self.p.clone()), replicas=[x.clone() for x in self.replicas],
                    m=self.m.clone(), v=self.v.clone(), before=self.before)


CLIP_T = torch.tensor(R.CLIP)


def life(world, mutant=None, epochs=R.EPOCHS):
    tr = StandIn(world, mutant)
    recs, n = [], 0
    for epoch in range(epochs):
        lr = E.lr_at(CFG, epoch)
        for s in range(R.STEPS):
            n += 1
            rec = tr.step(epoch, s, lr, n)
            rec.update(n=n, epoch=epoch, s=s, lr=lr)
            recs.append(rec)
    return recs


def judge(recs, clean, world):
    out, lines = {}, []
    for r, c in zip(recs, clean):
        tag = "step %d e%d s%d" % (r["n"], r["epoch"], r["s"])
        b = r["before"]
        ref = R.teacher_forced_dp_step(b["p"], b["m"], b["v"], r["n"] - 1, r["lr"],
                                       R.rank_inputs(NAME, world, r["epoch"], r["s"]), SC["H"], CFG["weight_decay"])
        fig = E.step_figures(r, ref)
        lines.append(E.figure_line(tag, fig, r["lr"], r["n"]))
        bad = E.broken_gates(fig, E.FP32_GATES, r["lr"], r["n"])
        if not all(torch.equal(x, r["replicas"][0]) for x in r["replicas"][1:]):
            bad.append("replicas")
        if not (r["loss"] == c["loss"] and r["norm"] == c["norm"] and torch.equal(r["replicas"][0], c["replicas"][0])
                and torch.equal(r["m"], c["m"]) and torch.equal(r["v"], c["v"])):
            bad.append("equal")
        out[tag] = bad
    return out, lines


_CLEAN = {}


def clean_run(world):
    if world not in _CLEAN:
        _CLEAN[world] = life(world)
    return _CLEAN[world]


@pytest.mark.parametrize("world", R.WORLDS)
def test_clean_stand_in_passes_every_gate(world):
    broken, lines = judge(clean_run(world), clean_run(world), world)
    print("\nclean f32 stand-in, FP32 script, world %d" % world)
    print("\n".join(lines))
    assert len(broken) == R.EPOCHS * R.STEPS and not any(broken.values()), broken


# (mutant, what it is, the step at which a gate must break)
MUTANTS = [
    ("stale_bucket", "rank 1's contribution to one bucket-sized range of decoder layer 1's FFN is step 1's", "step 2 e0 s1"),
    ("slot_collision", "ranks 1 and 2 land in the same slot of rank 0: rank 1's slice of that shard is lost", "step 2 e0 s1"),
    ("no_scale", "the loss gradient is not scaled by 1 / world", "step 2 e0 s1"),
    ("same_salt", "every rank draws its masks with salt 0", "step 2 e0 s1"),
    ("tail_unreduced", "the vector tail [n_shardable, numel) keeps rank 0's own gradients", "step 2 e0 s1"),
    ("norm_one_shard", "the clip norm comes from shard 0's partials (and the tail's) only", "step 2 e0 s1"),
    ("stale_peer_shard", "rank 1 keeps its old weights in rank 0's shard after the step", "step 2 e0 s1"),
]
ORACLE_GATES = ("grad", "pred", "loss", "norm", "param", "param_mean")


def test_each_mutant_breaks_a_gate_at_its_step():
    world = 3
    clean = clean_run(world)[:R.STEPS]
    rows, missed, loose = [], [], []
    for name, what, at in MUTANTS:
        broken, lines = judge(life(world, name, epochs=1), clean, world)
        first = next((tag for tag, bad in broken.items() if bad), None)
        rows.append((name, what, at, broken, first, next(x for x in lines if x.startswith(at))))
        if not broken[at] or first != at:
            missed.append(name)
        if not set(broken[at]) & set(ORACLE_GATES):
            loose.append(name)
    print("\nmutant table (FP32 script, world 3, the f32 stand-in; each mistake made at step 2)")
    for name, what, at, broken, first, line in rows:
        print("%-16s %-100s at %s breaks %s; step 3: %s" % (name, what, at, ",".join(broken[at]) or "NOTHING",
                                                           ",".join(broken["step 3 e0 s2"]) or "nothing"))
        print("    " + line)
    print("separated by the exact gates only: %s" % (", ".join(loose) or "none"))
    assert not missed, missed
    # a peer's stale weights are no part of the state the oracle is started from: at the step
    # itself only `replicas` sees them; the next step's prediction and gradients then do
    assert loose == ["stale_peer_shard"], loose
    late = dict((r[0], r[3]["step 3 e0 s2"]) for r in rows)["stale_peer_shard"]
    assert set(late) & set(ORACLE_GATES), late

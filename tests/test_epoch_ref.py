"""CPU proof of tests/epoch_ref.py, which tests/test_epoch_life_gpu.py judges a scripted
epoch by.  No GPU.

  * adam_ratio_bound: 1 at t = 1, never exceeded by 10^4 random and adversarial gradient
    sequences for t <= 8, attained by the Cauchy-Schwarz extremal sequence.
  * teacher_forced_step from a trainer's own state reproduces that trainer's next step
    exactly in float64.
  * Mutants.  An f32 CPU stand-in of the engine (OracleTrainer(dtype=float32) with its step
    restated so that single mistakes can be switched on) runs the FP32 script through
    both epochs and a checkpoint round trip.  Every event is judged as the GPU test
    judges run Y:
      oracle gates (3b)   each training step against teacher_forced_step from the run's
                          own parameters and moments before it, the step count and lr of
                          the script, the masks of the run's seed: grad, pred, loss,
                          norm, param, param_mean (epoch_ref.broken_gates); each
                          validation forward against seq2seq_forward in float64: val
      exact gates (3a)    what the GPU test asserts bit for bit and needs no kernel to
                          state: the seed of each training forward is that epoch's next
                          torch draw (seed), the step count before a step (count) and lr
                          (lr) are the script's, and the epoch after the checkpoint round
                          trip equals the uninterrupted one (resume)
    The clean run breaks none.  Each of the eight mutants breaks at least one at the
    step named, and the table printed says which (profiles/epoch_life_errors.txt).  The
    oracle gates alone separate seven of them.  They are too loose for one: moments that
    are zero after resume are invisible to teacher forcing by construction (the oracle
    starts from the run's own moments), so only `resume` separates that mutant.  Epoch 0's
    lr in epoch 1 and a step count restarting at 1 make the update wrong by a factor (2
    and 1.7), which the lr / 2 gate on a tensor's mean sees (0.67 lr, and 0.51 lr: by
    little); `lr`, `count` and `resume` see them whatever the oracle gates say."""
import numpy as np
import pytest
import torch

from oracle import model_ref
from tests import epoch_ref as E
from tests import step_ref as S

NAME = "FP32"
SC = E.SCRIPTS[NAME]
CFG = E.config(NAME)
N_TRAIN = len(SC["train"])


@pytest.fixture(scope="module", autouse=True)
def few_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(4, n))
    yield
    torch.set_num_threads(n)


# ---------------------------------------------------------------------------- the bound
def test_bound_is_one_at_the_first_step():
    assert E.adam_ratio_bound(1) == pytest.approx(1.0, abs=1e-15)
    assert E.adam_ratio_bound(2) == pytest.approx(1.0013, abs=1e-4)
    assert all(E.adam_ratio_bound(t + 1) > E.adam_ratio_bound(t) for t in range(1, 8))


def sequences(t, rng):
    """10^4 rows [n, t]: normal, heavy-tailed scales, near-extremal, and the adversarial
    families: constant, alternating, a single spike at each position, a sign flip at
    each position, geometric ramps around the extremal ratio."""
    n = 10000
    ext = np.array(E.extremal_sequence(t))
    rows = [rng.standard_normal((n // 4, t)),
            rng.standard_normal((n // 4, t)) * np.exp(4 * rng.standard_normal((n // 4, t))),
            ext * (1 + 0.1 * rng.standard_normal((n // 4, t))),
            ext * np.exp(rng.standard_normal((n // 4, 1)))]
    fixed = [np.ones(t), -np.ones(t), (-1.0) ** np.arange(t), ext, -ext, ext[::-1]]
    for i in range(t):
        spike = np.zeros(t)
        spike[i] = 1.0
        flip = np.ones(t)
        flip[i:] = -1.0
        small = np.full(t, 1e-6)
        small[i] = 1.0
        fixed += [spike, flip, small]
    for r in (0.5, 0.8, 0.9, 0.9009, 0.95, 1.0, 1.1, 2.0, 10.0):
        fixed.append(r ** np.arange(t)[::-1])
    return np.concatenate(rows + [np.array(fixed)])


@pytest.mark.parametrize("t", range(1, 9))
def test_bound_holds_and_is_attained(t):
    g = sequences(t, np.random.default_rng(100 + t))
    assert g.shape[0] >= 10000
    worst = np.abs(E.adam_ratio(g)).max()
    bound = E.adam_ratio_bound(t)
    print("t %d: bound %.6f, worst of %d sequences %.6f" % (t, bound, g.shape[0], worst))
    assert worst <= bound * (1 + 1e-12)
    assert E.adam_ratio(np.array([E.extremal_sequence(t)]))[0] >= 0.99 * bound


# ---------------------------------------------------------------------- teacher forcing
def test_teacher_forcing_reproduces_the_trainers_next_step():
    train, _ = E.batches(NAME)
    H = SC["H"]
    tr = model_ref.OracleTrainer(E.params(NAME), H, lr=CFG["learning_rate"], weight_decay=CFG["weight_decay"],
                                 dtype=torch.float64)
    seeds = E.epoch_seeds(0, 3)
    for i, (src, trg) in enumerate(train):
        masks = E.masks_of(NAME, src.shape[0], src.shape[1], seeds[i])
        tr.lr = E.lr_at(CFG, i % 2)  # both learning rates
        before = ({k: tr.p[k].detach().clone() for k in tr.keys}, dict(zip(tr.keys, [x.clone() for x in tr.m])),
                  dict(zip(tr.keys, [x.clone() for x in tr.v])), tr.step_count)
        ref = E.teacher_forced_step(*before, tr.lr, src, trg, masks, H, CFG["weight_decay"])
        loss, norm, pred = tr.step(src.double(), trg.double(), masks=masks)
        assert ref["loss"] == loss.item() and ref["norm"] == norm.item() and torch.equal(ref["pred"], pred)
        assert ref["step"] == tr.step_count == i + 1
        for j, k in enumerate(tr.keys):
            assert torch.equal(ref["grads"][k], tr.last_grads[k]), k
            assert torch.equal(ref["params"][k], tr.p[k].detach()), k
            assert torch.equal(ref["m"][k], tr.m[j]) and torch.equal(ref["v"][k], tr.v[j]), k


# ------------------------------------------------------------------------------ mutants
def stage_matrices(keys, stage):
    """The matrices of one forward stage (engine.update_ranges' stages)."""
    prefix = {"enc": "encoder.transformer_encoder.%d.", "dec": "decoder.transformer_decoder.%d."}[stage[0]] % stage[1]
    return [k for k in keys if k.startswith(prefix) and k.endswith(".weight") and ".norm" not in k]


class StandIn(model_ref.OracleTrainer):
    """OracleTrainer(float32) whose step is restated with one switch per mistake; with
    no switch it is OracleTrainer.step (test_stand_in_is_the_oracle_trainer)."""

    def __init__(self, params, mutant=None):
        super().__init__(params, SC["H"], lr=CFG["learning_rate"], weight_decay=CFG["weight_decay"], clip=E.CLIP,
                         dtype=torch.float32)
        self.mutant = mutant
        self.p_before_last_update = None
        self.arena_grads = None  # what the last backward left in the gradient arena (unclipped)
        self.prev_norm = None

    def step(self, src, trg, masks=None, n=0):
        """n: 1-based index of this training step in the whole run."""
        hit = lambda name, at: self.mutant == name and n == at
        leaves = dict(self.p)
        if hit("stale_forward", 2):
            for k in stage_matrices(self.keys, ("dec", 0)):
                leaves[k] = self.p_before_last_update[k].clone().requires_grad_(True)
        for k in self.keys:
            leaves[k].grad = None
        pred = model_ref.seq2seq_forward(leaves, src, self.num_heads, self.dropout, self.dropout > 0 or masks is not None,
                                         masks)
        loss = model_ref.loss_fn(pred, trg, *self.loss_args)
        loss.backward()
        grads = [leaves[k].grad for k in self.keys]
        if hit("accumulate", 3):
            grads = [g + self.arena_grads[k] for g, k in zip(grads, self.keys)]
        self.last_grads = {k: g.detach().clone() for k, g in zip(self.keys, grads)}
        self.arena_grads = self.last_grads
        with torch.no_grad():
            if hit("stale_norm", 3):
                total = self.prev_norm
                coef = torch.clamp(self.clip / (total + 1e-6), max=1.0)
                for g in grads:
                    g.mul_(coef)
            else:
                total = model_ref.clip_grad_norm(grads, self.clip)
            self.prev_norm = total
            self.step_count += 1
            self.p_before_last_update = {k: self.p[k].detach().clone() for k in self.keys}
            upd = list(range(len(self.keys)))
            if hit("skip_stage", 2):
                skip = set(stage_matrices(self.keys, ("enc", 1)))
                upd = [i for i in upd if self.keys[i] not in skip]
            model_ref.adam_l2_step([self.p[self.keys[i]] for i in upd], [grads[i] for i in upd],
                                   [self.m[i] for i in upd], [self.v[i] for i in upd], self.step_count, self.lr,
                                   weight_decay=self.wd)
        return loss.detach(), total, pred.detach()


def checkpoint_round_trip(tr, mutant):
    """A fresh stand-in from what a checkpoint holds of `tr`."""
    new = StandIn({k: tr.p[k].detach().clone() for k in tr.keys}, mutant)
    new.m, new.v = [x.clone() for x in tr.m], [x.clone() for x in tr.v]
    new.step_count = tr.step_count
    new.arena_grads, new.prev_norm, new.p_before_last_update = tr.arena_grads, tr.prev_norm, tr.p_before_last_update
    if mutant == "step_restart":
        new.step_count = 0
    if mutant == "moments_zero":
        new.m, new.v = [torch.zeros_like(x) for x in tr.m], [torch.zeros_like(x) for x in tr.v]
    return new


def life(mutant=None, resume=True):
    """The FP32 script on the stand-in: [record per event], in run order."""
    train, val = E.batches(NAME)
    tr = StandIn(E.params(NAME), mutant)
    recs, n = [], 0
    for epoch in range(SC["epochs"]):
        if epoch == 1 and resume:
            tr = checkpoint_round_trip(tr, mutant)
        tr.lr = E.lr_at(CFG, 0 if mutant == "old_lr" else epoch)
        torch.manual_seed(E.EPOCH_SEED + epoch)
        n_val = 0
        for kind, i in E.events(NAME):
            if kind == "train":
                n += 1
                src, trg = train[i]
                seed = S.salted_seed(int(torch.randint(0, 2 ** 62, (1,)).item()), 0)
                masks = E.masks_of(NAME, src.shape[0], src.shape[1], seed)
                before = dict(p={k: tr.p[k].detach().clone() for k in tr.keys},
                              m=dict(zip(tr.keys, [x.clone() for x in tr.m])),
                              v=dict(zip(tr.keys, [x.clone() for x in tr.v])), step=tr.step_count, lr=tr.lr)
                loss, norm, pred = tr.step(src, trg, masks=masks, n=n)
                recs.append(dict(kind="train", epoch=epoch, i=i, n=n, seed=seed, before=before, loss=loss.item(),
                                 norm=norm.item(), pred=pred, grads=tr.last_grads,
                                 params={k: tr.p[k].detach().clone() for k in tr.keys},
                                 m=[x.clone() for x in tr.m], v=[x.clone() for x in tr.v]))
            else:
                n_val += 1
                src, trg = val[i]
                p = {k: tr.p[k].detach().clone() for k in tr.keys}
                with torch.no_grad():
                    if mutant == "val_dropout" and epoch == 0 and n_val == 1:
                        seed = S.salted_seed(int(torch.randint(0, 2 ** 62, (1,)).item()), 0)
                        pred = model_ref.seq2seq_forward(p, src, SC["H"], SC["p"], True,
                                                         E.masks_of(NAME, src.shape[0], src.shape[1], seed))
                    else:
                        pred = model_ref.seq2seq_forward(p, src, SC["H"])
                    loss = model_ref.loss_fn(pred, trg).item()
                recs.append(dict(kind="val", epoch=epoch, i=i, n=n, params=p, pred=pred, loss=loss))
    return recs


def judge(recs, clean):
    """{event tag: [broken gates]} of a run, the events in run order; `clean`: the
    uninterrupted clean run (the `resume` gate compares epoch 1 with it bit for bit)."""
    train, val = E.batches(NAME)
    out, lines = {}, []
    want_seeds = {e: E.epoch_seeds(e, N_TRAIN) for e in range(SC["epochs"])}
    for r, c in zip(recs, clean):
        tag = "%s e%d %s%d" % ("step %d" % r["n"] if r["kind"] == "train" else "val after %d" % r["n"], r["epoch"],
                               "b" if r["kind"] == "train" else "v", r["i"])
        bad = []
        if r["kind"] == "train":
            src, trg = train[r["i"]]
            b = r["before"]
            lr, t = E.lr_at(CFG, r["epoch"]), r["n"]
            ref = E.teacher_forced_step(b["p"], b["m"], b["v"], t - 1, lr, src, trg,
                                        E.masks_of(NAME, src.shape[0], src.shape[1], r["seed"]), SC["H"],
                                        CFG["weight_decay"])
            fig = E.step_figures(r, ref)
            lines.append(E.figure_line(tag, fig, lr, t))
            bad += E.broken_gates(fig, E.FP32_GATES, lr, t)
            if r["seed"] != want_seeds[r["epoch"]][r["i"]]:
                bad.append("seed")
            if b["step"] != t - 1:
                bad.append("count")
            if b["lr"] != lr:
                bad.append("lr")
            if r["epoch"] == 1 and not (r["loss"] == c["loss"] and r["norm"] == c["norm"]
                                        and all(torch.equal(r["params"][k], c["params"][k]) for k in c["params"])
                                        and all(torch.equal(x, y) for x, y in zip(r["m"] + r["v"], c["m"] + c["v"]))):
                bad.append("resume")
        else:
            src, trg = val[r["i"]]
            e_pred, e_loss = E.val_figures(r["params"], src, trg, SC["H"], r["pred"], r["loss"])
            lines.append("%-28s pred %.2e loss %.2e" % (tag, e_pred, e_loss))
            if not (e_pred < E.VAL_GATE and e_loss < E.VAL_GATE):
                bad.append("val")
            if r["epoch"] == 1 and r["loss"] != c["loss"]:
                bad.append("resume")
        out[tag] = bad
    return out, lines


@pytest.fixture(scope="module")
def clean():
    return life(resume=False)


def test_stand_in_is_the_oracle_trainer():
    train, _ = E.batches(NAME)
    a = StandIn(E.params(NAME))
    b = model_ref.OracleTrainer(E.params(NAME), SC["H"], lr=CFG["learning_rate"], weight_decay=CFG["weight_decay"],
                                dtype=torch.float32)
    for n, (src, trg) in enumerate(train[:2]):
        masks = E.masks_of(NAME, src.shape[0], src.shape[1], 1000 + n)
        ra, rb = a.step(src, trg, masks=masks, n=n + 1), b.step(src, trg, masks=masks)
        assert all(torch.equal(x, y) for x, y in zip(ra, rb))
        assert all(torch.equal(a.p[k], b.p[k]) for k in a.keys)


def test_script_events_and_schedule():
    assert E.events("BF16") == [("train", 0), ("val", 0), ("train", 1), ("train", 2), ("val", 1), ("train", 3)]
    assert E.events("FP32") == [("train", 0), ("val", 0), ("train", 1), ("train", 2), ("val", 1)]
    assert E.events("FP8") == [("train", 0), ("val", 0), ("train", 1), ("val", 0), ("train", 2), ("val", 0)]
    for name in E.SCRIPTS:
        cfg = E.config(name)
        assert E.lr_at(cfg, 0) == cfg["learning_rate"] and E.lr_at(cfg, 1) == 0.5 * cfg["learning_rate"]
    assert len(set(E.epoch_seeds(0, 4) + E.epoch_seeds(1, 4))) == 8


def test_clean_stand_in_passes_every_gate(clean):
    resumed = life(resume=True)
    broken, lines = judge(resumed, clean)
    print("\nclean f32 stand-in, FP32 script, through the checkpoint round trip")
    print("\n".join(lines))
    assert not any(broken.values()), broken


# (mutant, what it is, the event at which a gate must break)
MUTANTS = [
    ("skip_stage", "encoder layer 1's matrices not updated at step 2", "step 2 e0 b1"),
    ("stale_forward", "decoder layer 0's forward of step 2 reads the weights from before step 1's update",
     "step 2 e0 b1"),
    ("accumulate", "the partial-batch step 3 accumulates onto step 2's gradients", "step 3 e0 b2"),
    ("stale_norm", "step 3 clips with step 2's norm", "step 3 e0 b2"),
    ("old_lr", "epoch 0's lr used in epoch 1", "step 4 e1 b0"),
    ("step_restart", "the step count restarts at 1 after resume", "step 4 e1 b0"),
    ("moments_zero", "the moments are zero after resume", "step 4 e1 b0"),
    ("val_dropout", "the first validation forward runs with dropout on (and draws a seed)", "val after 1 e0 v0"),
]
ORACLE_GATES = ("grad", "pred", "loss", "norm", "param", "param_mean", "val")


def test_each_mutant_breaks_a_gate_at_its_step(clean):
    rows, missed, loose = [], [], []
    for name, what, at in MUTANTS:
        broken, lines = judge(life(name), clean)
        first = next((tag for tag, bad in broken.items() if bad), None)
        rows.append((name, what, at, broken[at], first, next(x for x in lines if x.startswith(at))))
        if not broken[at]:
            missed.append(name)
        if not set(broken[at]) & set(ORACLE_GATES):
            loose.append(name)
    print("\nmutant table (FP32 script on the f32 stand-in)")
    for name, what, at, bad, first, line in rows:
        print("%-14s %-84s at %-18s breaks %s%s" % (name, what, at, ",".join(bad) or "NOTHING",
                                                     "" if first == at else "  (first broken event: %s)" % first))
        print("    " + line)
    print("separated by the exact gates only (the oracle gates are too loose for them): %s" % (", ".join(loose) or "none"))
    assert not missed, missed
    # moments_zero cannot move an oracle that starts from the run's own moments
    # step_restart clears the lr / 2 gate on a tensor's mean by little (0.512 lr): `count` is its gate
    assert "moments_zero" in loose and not set(loose) - {"moments_zero", "step_restart"}, loose

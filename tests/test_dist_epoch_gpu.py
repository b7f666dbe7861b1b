"""A scripted multi-rank epoch through training_utils.train_one_epoch_multi_gpu itself, two
and three ranks on one card (gloo carries the collectives, every rank on cuda:0, as
tests/test_dist_gpu.py), with the gradient buckets cut small so that the in-backward
exchange really launches.  tests/dist_ref.py has the scripts, the float64 reference and the
arena's ready sites; tests/test_dist_ref.py proves them on the CPU and shows seven mistakes
of the kind looked for here breaking the gates below.

The default bucket (parallel.DEFAULT_BUCKET_BYTES, 16.7 M f32) is larger than any test
model's arena: with it reducer.ready never launches and every byte moves in finish(), after
the whole backward.  The small bucket (dist_ref.small_bucket: 15000 elements for the BF16
script, 7000 for FP32) is below the smallest growth of the final prefix between two ready
call sites of engine.backward and divides no shard, so every ready call releases buckets and
their edges fall inside layers, inside the cross-attention k|v block and across shard
boundaries.  A bucket released before its last writer was enqueued carries the previous
step's gradient (or a deferred launch's missing one): nothing crashes, and only equality
with a run that exchanged after the whole backward shows it.

A worker builds the model from dist_ref's seeded parameters, attaches data parallelism
itself, sets the bucket, and runs the loop once per epoch; between epochs, as
train.train_model: scheduler.step(), optimizer.consolidate(), rank 0's save_checkpoint, a
barrier.  print_training_progress, _validation_step, the criterion, engine.draw_seed and the
reducer's begin / ready / finish are wrapped to record; the loop's own code runs.

Gates
 1  world 2, bit for bit: zero1_push small and zero1_overlap small equal zero1; allreduce
    small equals allreduce default (two-term sums commute): every loss, clip norm and
    validation loss, and after each epoch every parameter, both moments and the step count.
 2  world 3, bit for bit: zero1_push small equals zero1_push default (nstl_shard_sum adds
    own + slots in rank order whatever the bucket).
 3  replicas: every rank's p16[:n_shardable] before consolidate() and every rank's
    consolidated state after it are bit-identical.
 4  rank 0's validation forward between sharded steps leaves eng.p16 as it was (its f32
    masters outside its shard are stale then: a refresh_shadow would show).
 5  the epoch resumed from rank 0's checkpoint equals the original epoch 1, bit for bit.
 6  allreduce against zero1_push at world 2: parameters within rtol 1e-5, atol 1e-6 and clip
    norms within 1e-4 (tests/test_dist_gpu.py's), only the norm's reduction order differs.
 7  against the float64 oracle, teacher-forced from the run's own state (each rank's own
    shard of the masters and moments is cloned after a step, in stream order, no collective
    and no host sync: together they are the consolidated state): FP32 at worlds 2 and 3 every
    training step and every validation forward, BF16 zero1_push step 1 of each epoch; gates
    epoch_ref.FP32_GATES / BF16_GATES / VAL_GATE and the derived Adam bound, as
    tests/test_epoch_life_gpu.py applies them.
 C  NSTL_DP=allreduce with FusedAdam.overlap_next_forward (as bench.py sets it at every world
    size): normal steps equal the flag-off run, and so does a step over gradients written by
    hand (a different tensor per rank, no backward): the overlapped branch must not step on
    gradients no all-reduce finished.

With NSTL_PARITY_ERRORS_OUT=<file> the largest measured error of each figure is written next
to its gate, and each spawn's wall time (profiles/dist_epoch_errors.txt is such a run)."""
import datetime
import os
import shutil
import socket
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import dist_ref as R
from tests import epoch_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COLLECTIVE_TIMEOUT_S = 90
PUSH_TIMEOUT_S = 15
SHARDED = ("zero1", "zero1_push", "zero1_overlap")

_ERRORS = {}   # figure -> (fraction of the gate used, gate, measured)
_SPAWN_S = {}  # run -> wall seconds of its mp.spawn
_BROKEN = []


def _note(what, measured, gate):
    frac = measured / gate
    if what not in _ERRORS or frac > _ERRORS[what][0]:
        _ERRORS[what] = (frac, "%.3e" % gate, "%.3e" % measured)


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    t0 = time.monotonic()
    yield
    path = os.environ.get("NSTL_PARITY_ERRORS_OUT")
    if path and _ERRORS:
        with open(path, "w") as f:
            f.write("# tests/test_dist_epoch_gpu.py: largest measured error of each figure next to its gate\n")
            f.write("# %-38s %-14s %-14s %s\n" % ("figure", "gate", "measured", "measured / gate"))
            for what in sorted(_ERRORS):
                frac, gate, measured = _ERRORS[what]
                f.write("%-40s %-14s %-14s %.4f\n" % (what, gate, measured, frac))
            f.write("# wall seconds of each spawn (process start, import, model build, %d steps, dumps)\n"
                    % (R.EPOCHS * R.STEPS))
            for what, s in _SPAWN_S.items():
                f.write("spawn %-50s %.1f\n" % (what, s))
            f.write("module wall seconds %.1f, %d spawns, %.1f s per spawn\n"
                    % (time.monotonic() - t0, len(_SPAWN_S), sum(_SPAWN_S.values()) / max(1, len(_SPAWN_S))))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _join(rank, port, world, mode):
    """The process group of a worker: gloo with a bounded timeout, initialised here."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", NSTL_DP=mode, NSTL_PUSH_TIMEOUT_S=str(PUSH_TIMEOUT_S))
    if mode == "zero1_overlap":
        os.environ["NSTL_CEDE_CUS"] = "0"  # gloo: no collective kernel is resident, nothing to cede CUs to
    from neurosync_trainer_lite_amd import parallel
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=COLLECTIVE_TIMEOUT_S))
    assert parallel.init_from_env(backend="gloo") == (rank, world, 0)


def _components(name):
    from neurosync_trainer_lite_amd.utils.model_utils import build_model, prepare_training_components
    cfg = R.config(name)
    model = build_model(cfg, DEV)
    crit, opt, sched = prepare_training_components(cfg, model)
    return cfg, model, crit, opt, sched


def _build_engine(model, src):
    model.eval()
    with torch.no_grad():
        model(src.to(DEV))  # builds the engine's buffers; an eval forward draws no seed
    model.train()
    return model.engine()


def _record_reducer(red, backs):
    """begin / ready / finish of `red` wrapped: one record per backward, `sent` before and
    after each ready call and what finish() was left with."""
    real_begin, real_ready, real_finish = red.begin, red.ready, red.finish

    def begin(fresh):
        real_begin(fresh)
        backs.append(dict(ready=[], sent_at_finish=None))

    def ready(upto):
        before = red.sent
        real_ready(upto)
        backs[-1]["ready"].append((int(upto), int(before), int(red.sent)))

    def finish():
        backs[-1]["sent_at_finish"] = int(red.sent)
        real_finish()

    red.begin, red.ready, red.finish = begin, ready, finish


# ------------------------------------------------------------------------------ the worker
def _epoch_worker(rank, port, out_dir, name, mode, world, bucket, resume, dump_steps):
    """bucket: elements, or None (the default).  resume: a checkpoint path, or None.
    dump_steps: the 1-based training steps after which this rank's shard of the state, the
    reduced gradients and the step's prediction are kept for the oracle."""
    _join(rank, port, world, mode)
    from neurosync_trainer_lite_amd import parallel
    from neurosync_trainer_lite_amd.train import _NoScaler
    from neurosync_trainer_lite_amd.utils import checkpoint_utils, training_utils
    work = os.path.join(out_dir, "rank%d" % rank)
    os.makedirs(work)
    os.chdir(work)  # the plots and the checkpoint land here
    lay = R.layout(name)
    train, val = R.batches(name, world)
    cfg, model, crit, opt, sched = _components(name)
    first, batch_step = 0, 0
    if resume is None:
        model.load_state_dict(R.params(name), strict=True)
    else:
        epoch0, batch_step, model, opt, sched = checkpoint_utils.load_checkpoint(resume, model, opt, sched,
                                                                                 torch.device(DEV))
        first = epoch0 + 1
        assert batch_step == first * R.STEPS
    eng = _build_engine(model, val[0][0])
    training_utils.attach_data_parallel(model, opt, world)
    assert eng.offsets == lay.offsets and (eng.n_shardable, eng.numel) == (lay.n_shardable, lay.numel)
    assert eng.end_of == lay.end_of
    assert eng.grad_scale_t.item() == torch.tensor(1.0 / world, dtype=torch.float32).item() and eng.seed_salt == rank
    ns = eng.n_shardable
    red = eng.grad_reducer
    assert (opt._comm is not None) == (mode in SHARDED)
    backs = []
    if mode == "zero1":
        assert red is None
    else:
        assert red is not None and red.active and red.mode == mode, (mode, red)
        if bucket is not None:
            red.bucket = bucket
        _record_reducer(red, backs)
    lo, hi = (opt._comm.lo, opt._comm.hi) if opt._comm is not None else (0, ns)

    rec, log, seeds, snaps = {}, dict(train=[], val=[]), [], {}
    real_draw = eng.draw_seed

    def draw_seed():
        s = real_draw()
        if eng.p > 0:
            seeds.append(s)
        return s
    eng.draw_seed = draw_seed

    def criterion(pred, trg, **kw):
        loss = crit(pred, trg, **kw)
        if dump_steps:
            log["train" if kw else "val"].append(pred.detach().clone())
        return loss

    real_step = opt.step

    def step(*a, **kw):
        out = real_step(*a, **kw)
        n = opt._nstl_step
        if n in dump_steps:
            g = opt._gs if opt._comm is not None else eng.g32[:ns]
            snaps[n] = dict(g=g.clone(), gt=eng.g32[ns:].clone(), pred=log["train"][-1],
                            **{k: t[lo:hi].clone() for k, t in (("p", eng.p32), ("m", opt.m), ("v", opt.v))},
                            **{k + "t": t[ns:].clone() for k, t in (("p", eng.p32), ("m", opt.m), ("v", opt.v))})
        return out
    opt.step = step

    def progress(batch_idx, total_norm, batch_loss, batch_step, epoch, total_epochs, dataloader_len, pbar):
        assert (batch_idx, dataloader_len, total_epochs) == (len(rec["steps"]), R.STEPS, cfg["n_epochs"])
        rec["steps"].append((batch_loss, total_norm))
        rec["lrs"].append(opt.param_groups[0]["lr"])

    real_val = training_utils._validation_step

    def validation(model_, val_iter, val_dl, crit_, device):
        assert rank == 0
        before, stale = eng.p16.clone(), bool(eng.master_stale)
        r = real_val(model_, val_iter, val_dl, crit_, device)
        rec["vals"].append(r[1])
        rec["val_same"].append(bool(torch.equal(before, eng.p16)))
        rec["val_stale"].append(stale)
        if dump_steps and eng.p16 is eng.p32:  # f32: the gathered weights are the masters
            rec["val_params"].append(eng.p32.cpu().clone())
            rec["val_preds"].append(log["val"][-1].cpu())
        assert model_.training
        return r

    training_utils.print_training_progress = progress
    training_utils._validation_step = validation
    epochs = []
    for epoch in range(first, R.EPOCHS):
        rec = dict(steps=[], lrs=[], vals=[], val_same=[], val_stale=[], val_params=[], val_preds=[])
        del seeds[:]
        torch.manual_seed(R.EPOCH_SEED + epoch)
        batch_step = training_utils.train_one_epoch_multi_gpu(
            epoch, [model], train, criterion, opt, [torch.device(DEV)], clip=R.CLIP, batch_step=batch_step, pbar=None,
            total_epochs=cfg["n_epochs"], use_amp=cfg["use_amp"], grad_scaler=_NoScaler() if cfg["use_amp"] else None,
            val_dataloader=val, validation_interval=R.INTERVAL)
        assert batch_step == opt._nstl_step == (epoch + 1) * R.STEPS  # the leftover batch made no step
        torch.cuda.synchronize()
        rec.update(seeds=list(seeds), p16=eng.p16[:ns].cpu().clone(), p16_tail=eng.p16[ns:].cpu().clone())
        sched.step()
        opt.consolidate()
        if rank == 0:
            checkpoint_utils.save_checkpoint(model, opt, sched, epoch, batch_step, cfg)
            shutil.copy(cfg["checkpoint_path"], os.path.join(out_dir, "after_epoch_%d.pth" % epoch))
        dist.barrier()
        torch.cuda.synchronize()
        rec.update(sd={k: v.cpu().clone() for k, v in model.state_dict().items()}, m=opt.m.cpu().clone(),
                   v=opt.v.cpu().clone(), step=opt._nstl_step,
                   osd_steps=sorted({float(s["step"]) for s in opt.state_dict()["state"].values()}))
        epochs.append(rec)
    # a silent fallback to zero1 would make every comparison with zero1 vacuous
    assert training_utils.gradient_exchange(model, opt) == mode, training_utils.gradient_exchange(model, opt)
    assert opt.dp_fallback is None, opt.dp_fallback
    if mode == "zero1_push":
        assert opt.dp_check is not None and opt.dp_check["ok"], opt.dp_check
    torch.save(dict(epochs=epochs, backs=backs, check=opt.dp_check, lo=lo, hi=hi,
                    snaps={n: {k: t.cpu() for k, t in s.items()} for n, s in snaps.items()}),
               os.path.join(out_dir, "r%d.pt" % rank))
    if hasattr(red, "close"):
        red.close()
    dist.destroy_process_group()


# ---------------------------------------------------------------------------------- runs
def _spawn(fn, args, world, what):
    """One spawn at a time, none after one that failed (a rank that died, a timeout): what
    failed on the card is not started again by the tests that share it."""
    if _BROKEN:
        pytest.fail("not started: an earlier spawn of this module failed (%s)" % _BROKEN[0])
    assert world <= 3
    t0 = time.monotonic()
    try:
        mp.spawn(fn, args=args, nprocs=world, join=True)
    except BaseException:
        _BROKEN.append(what)
        raise
    _SPAWN_S[what] = time.monotonic() - t0


ORACLE_DUMPS = {"FP32": tuple(range(1, R.EPOCHS * R.STEPS + 1)), "BF16": (1, R.STEPS + 1)}
_RUNS = {}


def run_of(tmp_path_factory, name, mode, world, kind):
    """kind: "small" | "default" | "resume" (small bucket, epoch 1 only, from rank 0's
    checkpoint of the small run's epoch 0).  Spawned once per module.  Rank 0's records are
    kept whole; of the other ranks' end states only whether they equal rank 0's."""
    key = (name, mode, world, kind)
    if key in _RUNS:
        return _RUNS[key]
    bucket = None if kind == "default" or mode == "zero1" else R.small_bucket(R.layout(name))
    resume = None
    if kind == "resume":
        resume = os.path.join(run_of(tmp_path_factory, name, mode, world, "small")["dir"], "after_epoch_0.pth")
    dumps = ORACLE_DUMPS[name] if (mode, kind) == ("zero1_push", "small") else ()
    what = "%s %s world %d %s" % key
    out = str(tmp_path_factory.mktemp("dist_%s_%s_%d_%s" % key))
    _spawn(_epoch_worker, (_port(), out, name, mode, world, bucket, resume, dumps), world, what)
    ranks = []
    for r in range(world):
        path = os.path.join(out, "r%d.pt" % r)
        ranks.append(torch.load(path, weights_only=True))
        os.unlink(path)
    r0 = ranks[0]
    agree = []
    for e, ep in enumerate(r0["epochs"]):
        row = dict(p16=True, tail=True, state=True, step=True)
        for other in ranks[1:]:
            oe = other["epochs"][e]
            row["p16"] &= torch.equal(ep["p16"], oe["p16"])
            row["tail"] &= torch.equal(ep["p16_tail"], oe["p16_tail"])
            row["state"] &= (all(torch.equal(ep["sd"][k], oe["sd"][k]) for k in ep["sd"])
                             and torch.equal(ep["m"], oe["m"]) and torch.equal(ep["v"], oe["v"]))
            row["step"] &= ep["step"] == oe["step"] and ep["osd_steps"] == oe["osd_steps"]
            for k in ("sd", "m", "v", "p16", "p16_tail"):
                del oe[k]
        agree.append(row)
    _RUNS[key] = dict(key=key, dir=out, ranks=ranks, epochs=r0["epochs"], agree=agree, bucket=bucket, world=world,
                      name=name, mode=mode)
    return _RUNS[key]


SMALL_RUNS = [("BF16", "zero1_push", 2), ("BF16", "zero1_overlap", 2), ("BF16", "allreduce", 2), ("BF16", "zero1_push", 3),
              ("FP32", "zero1_push", 2), ("FP32", "zero1_push", 3)]
ALL_RUNS = [k + ("small",) for k in SMALL_RUNS] + [("BF16", "zero1", 2, "small"), ("BF16", "allreduce", 2, "default"),
                                                   ("BF16", "zero1_push", 3, "default")]


def same_epoch(a, b, what):
    """Bit for bit: losses, norms, validation losses, parameters, moments, step count."""
    assert a["steps"] == b["steps"], (what, a["steps"], b["steps"])
    assert a["vals"] == b["vals"], (what, a["vals"], b["vals"])
    assert a["step"] == b["step"] and a["osd_steps"] == b["osd_steps"] == [float(a["step"])], (what, a["step"], b["step"])
    for k in a["sd"]:
        assert torch.equal(a["sd"][k], b["sd"][k]), (what, k, (a["sd"][k] - b["sd"][k]).abs().max().item())
    assert torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"]), what


def show(run):
    print("\n%s %s world %d %s, bucket %s" % (run["key"] + (run["bucket"],)))
    for r in run["epochs"]:
        print("  (loss, clip norm) %s  validation %s  step count %d" % (["(%.9g, %.9g)" % s for s in r["steps"]],
                                                                       ["%.9g" % v for v in r["vals"]], r["step"]))


# ---------------------------------------------------------- the launch assertions of a run
@pytest.mark.parametrize("name,mode,world,kind", ALL_RUNS)
def test_script_ran_and_buckets_left_at_every_ready_site(name, mode, world, kind, tmp_path_factory):
    run = run_of(tmp_path_factory, name, mode, world, kind)
    show(run)
    cfg, lay = R.config(name), R.layout(name)
    assert len(run["epochs"]) == R.EPOCHS
    for e, ep in enumerate(run["epochs"]):
        assert len(ep["steps"]) == R.STEPS and len(ep["vals"]) == sum(k == "val" for k, _ in R.events())
        assert all(x == x for s in ep["steps"] for x in s) and all(x == x for x in ep["vals"])  # no NaN
        assert ep["lrs"] == [E.lr_at(cfg, e)] * R.STEPS and ep["step"] == (e + 1) * R.STEPS
        for r, rank in enumerate(run["ranks"]):
            # every rank drew the same torch numbers, salted with its rank; none for a validation forward
            assert rank["epochs"][e]["seeds"] == R.rank_seeds(e, r), (e, r)
    if mode == "zero1":
        return
    sites = [end for _, end in R.ready_sites(lay)]
    target = lay.numel if mode == "allreduce" else lay.n_shardable
    for rank in run["ranks"]:
        assert len(rank["backs"]) == R.EPOCHS * R.STEPS
        for b in rank["backs"]:
            assert [u for u, _, _ in b["ready"]] == sites, b["ready"]
            if kind == "default":
                # the default bucket: nothing leaves before finish(), but a whole shard once it is final
                # (the sharded exchanges cut their buckets at shard boundaries)
                shard = lay.n_shardable // world if mode in SHARDED else target + 1
                assert all(after == upto // shard * shard for upto, _, after in b["ready"]), b["ready"]
                continue
            prev = 0
            for upto, before, after in b["ready"]:
                if upto > prev:
                    assert after > before and upto - run["bucket"] < after <= upto, (upto, before, after)
                prev = max(prev, upto)
            assert 0 < target - b["sent_at_finish"] < R.smallest_layer(lay), (target, b["sent_at_finish"])


# ------------------------------------------------------------------------------ gates 1, 2
@pytest.mark.parametrize("mode", ["zero1_push", "zero1_overlap"])
def test_world2_small_bucket_exchange_equals_zero1(mode, tmp_path_factory):
    a = run_of(tmp_path_factory, "BF16", "zero1", 2, "small")
    b = run_of(tmp_path_factory, "BF16", mode, 2, "small")
    for e in range(R.EPOCHS):
        same_epoch(a["epochs"][e], b["epochs"][e], "zero1 against %s small, epoch %d" % (mode, e))


def test_world2_allreduce_small_bucket_equals_default(tmp_path_factory):
    a = run_of(tmp_path_factory, "BF16", "allreduce", 2, "default")
    b = run_of(tmp_path_factory, "BF16", "allreduce", 2, "small")
    for e in range(R.EPOCHS):
        same_epoch(a["epochs"][e], b["epochs"][e], "allreduce default against small, epoch %d" % e)


def test_world3_push_small_bucket_equals_default(tmp_path_factory):
    a = run_of(tmp_path_factory, "BF16", "zero1_push", 3, "default")
    b = run_of(tmp_path_factory, "BF16", "zero1_push", 3, "small")
    for e in range(R.EPOCHS):
        same_epoch(a["epochs"][e], b["epochs"][e], "zero1_push default against small at world 3, epoch %d" % e)


# ------------------------------------------------------------------------------ gates 3, 4
@pytest.mark.parametrize("name,mode,world,kind", ALL_RUNS)
def test_replicas_agree_and_validation_leaves_the_weights(name, mode, world, kind, tmp_path_factory):
    run = run_of(tmp_path_factory, name, mode, world, kind)
    for e, (row, ep) in enumerate(zip(run["agree"], run["epochs"])):
        assert row["p16"], "p16[:n_shardable] differs between ranks before consolidate(), epoch %d" % e
        assert row["tail"] and row["state"] and row["step"], (e, row)
        assert ep["val_same"] == [True] * len(ep["vals"]), ep["val_same"]
        if mode in SHARDED and name == "BF16":
            # the condition under which a refresh_shadow would have overwritten gathered weights
            assert ep["val_stale"] == [True] * len(ep["vals"]), ep["val_stale"]


# --------------------------------------------------------------------------------- gate 5
def test_epoch_resumed_from_rank0_checkpoint_equals_the_run(tmp_path_factory):
    x = run_of(tmp_path_factory, "BF16", "zero1_push", 2, "small")
    r = run_of(tmp_path_factory, "BF16", "zero1_push", 2, "resume")
    show(r)
    assert len(r["epochs"]) == 1 and r["epochs"][0]["lrs"] == x["epochs"][1]["lrs"]
    same_epoch(x["epochs"][1], r["epochs"][0], "epoch 1 against the resumed epoch 1")
    assert r["agree"][0]["p16"] and r["agree"][0]["state"]
    ck = torch.load(os.path.join(x["dir"], "after_epoch_1.pth"), map_location="cpu", weights_only=True)
    assert (ck["epoch"], ck["batch_step"]) == (1, x["epochs"][1]["step"])
    for k, v in ck["model_state_dict"].items():
        assert torch.equal(v, x["epochs"][1]["sd"][k]), k


# --------------------------------------------------------------------------------- gate 6
def test_allreduce_agrees_with_push_at_world2(tmp_path_factory):
    a = run_of(tmp_path_factory, "BF16", "allreduce", 2, "small")
    b = run_of(tmp_path_factory, "BF16", "zero1_push", 2, "small")
    for e in range(R.EPOCHS):
        ea, eb = a["epochs"][e], b["epochs"][e]
        for k in ea["sd"]:
            d = (ea["sd"][k] - eb["sd"][k]).abs()
            _note("allreduce vs push: parameter", (d / (1e-6 + 1e-5 * eb["sd"][k].abs())).max().item(), 1.0)
            torch.testing.assert_close(ea["sd"][k], eb["sd"][k], rtol=1e-5, atol=1e-6)
        for (_, na), (_, nb) in zip(ea["steps"], eb["steps"]):
            _note("allreduce vs push: clip norm", abs(na - nb) / nb, 1e-4)
            assert abs(na - nb) < 1e-4 * nb, (na, nb)


# --------------------------------------------------------------------------------- gate 7
def _arena(run, n, key):
    """The arena `key` (p, m, v: the state after step n; g: step n's reduced gradients)
    from every rank's own shard and rank 0's tail."""
    lay = R.layout(run["name"])
    parts = [rank["snaps"][n][key] for rank in run["ranks"]]
    assert [rank["lo"] for rank in run["ranks"]] == [r * parts[0].numel() for r in range(run["world"])]
    tails = [rank["snaps"][n][key + "t"] for rank in run["ranks"]]
    assert all(torch.equal(t, tails[0]) for t in tails[1:]), "the replicated tail differs between ranks (%s)" % key
    out = torch.cat(parts + [tails[0]])
    assert out.numel() == lay.numel
    return R.unflat(lay, out)


def _oracle_step(run, n):
    name, world = run["name"], run["world"]
    sc, cfg = R.SCRIPTS[name], R.config(name)
    epoch, s = divmod(n - 1, R.STEPS)
    if s > 0:
        before = {k: _arena(run, n - 1, k) for k in ("p", "m", "v")}
    elif epoch == 0:
        p = R.params(name)
        before = dict(p=p, m={k: torch.zeros_like(x) for k, x in p.items()}, v={k: torch.zeros_like(x) for k, x in p.items()})
    else:
        lay, ep = R.layout(name), run["epochs"][epoch - 1]
        before = dict(p=ep["sd"], m=R.unflat(lay, ep["m"]), v=R.unflat(lay, ep["v"]))
    lr = E.lr_at(cfg, epoch)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    ref = R.teacher_forced_dp_step(before["p"], before["m"], before["v"], n - 1, lr, R.rank_inputs(name, world, epoch, s),
                                   sc["H"], cfg["weight_decay"])
    loss, norm = run["epochs"][epoch]["steps"][s]
    got = dict(loss=loss, norm=norm, pred=torch.cat([rank["snaps"][n]["pred"].reshape(-1, R.OUT_DIM) for rank in run["ranks"]]),
               grads=_arena(run, n, "g"), params=_arena(run, n, "p"))
    ref["pred"] = ref["pred"].reshape(-1, R.OUT_DIM)
    fig = E.step_figures(got, ref)
    tag = "%s world %d" % (name, world)
    print("\n" + E.figure_line("%s step %d e%d s%d" % (tag, n, epoch, s), fig, lr, n))
    gates = R.GATES[name]
    for k in ("grad", "loss", "norm"):
        _note("%s: %s" % (tag, k), fig[k], gates[k])
    _note("%s: pred" % tag, fig["pred_close"] if gates["pred_allclose"] else fig["pred"], gates["pred"])
    _note("%s: parameter step / lr" % tag, max(fig["step_err"], 0.0) / lr, 2 * E.adam_ratio_bound(n))
    _note("%s: tensor mean step / lr" % tag, fig["mean_step"] / lr, 0.5)
    return E.broken_gates(fig, gates, lr, n), fig


@pytest.mark.parametrize("n", ORACLE_DUMPS["FP32"])
@pytest.mark.parametrize("world", R.WORLDS)
def test_fp32_steps_match_the_data_parallel_oracle(world, n, tmp_path_factory):
    bad, fig = _oracle_step(run_of(tmp_path_factory, "FP32", "zero1_push", world, "small"), n)
    assert not bad, (bad, fig)


@pytest.mark.parametrize("n", ORACLE_DUMPS["BF16"])
@pytest.mark.parametrize("world", R.WORLDS)
def test_bf16_first_steps_match_the_data_parallel_oracle(world, n, tmp_path_factory):
    bad, fig = _oracle_step(run_of(tmp_path_factory, "BF16", "zero1_push", world, "small"), n)
    assert not bad, (bad, fig)


@pytest.mark.parametrize("world", R.WORLDS)
def test_fp32_validation_forwards_match_the_oracle(world, tmp_path_factory):
    run = run_of(tmp_path_factory, "FP32", "zero1_push", world, "small")
    lay, sc = R.layout("FP32"), R.SCRIPTS["FP32"]
    val = R.batches("FP32", world)[1]
    vals = [j for kind, j in R.events() if kind == "val"]
    bad = []
    print()
    for e, ep in enumerate(run["epochs"]):
        assert len(ep["val_params"]) == len(vals)
        for j, params, pred, loss in zip(vals, ep["val_params"], ep["val_preds"], ep["vals"]):
            src, trg = val[j]
            e_pred, e_loss = E.val_figures(R.unflat(lay, params), src, trg, sc["H"], pred, loss)
            print("FP32 world %d e%d v%d   pred %.2e loss %.2e" % (world, e, j, e_pred, e_loss))
            _note("FP32 world %d: validation pred" % world, e_pred, E.VAL_GATE)
            _note("FP32 world %d: validation loss" % world, e_loss, E.VAL_GATE)
            if not (e_pred < E.VAL_GATE and e_loss < E.VAL_GATE):
                bad.append((e, j, e_pred, e_loss))
    assert not bad, bad


# ------------------------------------------------- C: the overlapped update beside a reducer
def _overlap_worker(rank, port, out_dir, overlap):
    world, name = 2, "BF16"
    _join(rank, port, world, "allreduce")
    from neurosync_trainer_lite_amd import parallel
    from neurosync_trainer_lite_amd.utils import training_utils
    train, val = R.batches(name, world)
    cfg, model, crit, opt, sched = _components(name)
    model.load_state_dict(R.params(name), strict=True)
    eng = _build_engine(model, val[0][0])
    training_utils.attach_data_parallel(model, opt, world)
    red = eng.grad_reducer
    assert isinstance(red, parallel.GradAllReducer) and red.active and opt._comm is None
    red.bucket = R.small_bucket(R.layout(name))
    opt.overlap_next_forward = overlap  # as bench.py sets it at every world size
    assert opt._overlap_allowed
    torch.manual_seed(R.EPOCH_SEED)
    out = dict(norms=[], queued=[])

    def normal_step(s):
        src, trg = train[s * world + rank]
        opt.zero_grad()
        crit(model(src.to(DEV)), trg.to(DEV)).backward()
        opt.step(max_norm=R.CLIP)
        out["norms"].append(opt.last_norm)
        out["queued"].append(len(eng._wpending))

    def state(tag):
        opt._sync()
        torch.cuda.synchronize()
        out[tag] = dict(sd={k: v.cpu().clone() for k, v in model.state_dict().items()}, m=opt.m.cpu().clone(),
                        v=opt.v.cpu().clone())
    normal_step(0)
    normal_step(1)
    state("normal")
    # gradients written by hand, a different tensor per rank, no backward before the step
    # (the arena's padding stays zero, as every backward leaves it)
    gen = torch.Generator().manual_seed(900 + rank)
    hand = R.flat(R.layout(name), {k: torch.randn(shp, generator=gen) * 1e-3 for k, shp in R.shapes(name).items()})
    eng.g32.copy_(hand.to(DEV))
    opt.step(max_norm=R.CLIP)
    out["norms"].append(opt.last_norm)
    out["queued"].append(len(eng._wpending))
    state("hand")
    normal_step(2)
    state("after")
    out["norms"] = [float(x.item()) for x in out["norms"]]
    torch.save(out, os.path.join(out_dir, "c%d.pt" % rank))
    dist.destroy_process_group()


_C = {}


def c_run(tmp_path_factory, overlap):
    if overlap not in _C:
        out = str(tmp_path_factory.mktemp("overlap_%d" % overlap))
        _spawn(_overlap_worker, (_port(), out, overlap), 2, "C allreduce world 2 overlap %s" % overlap)
        _C[overlap] = [torch.load(os.path.join(out, "c%d.pt" % r), weights_only=True) for r in range(2)]
    return _C[overlap]


def _same_state(a, b, what):
    for k in a["sd"]:
        assert torch.equal(a["sd"][k], b["sd"][k]), (what, k, (a["sd"][k] - b["sd"][k]).abs().max().item())
    assert torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"]), what


def test_overlapped_update_beside_a_reducer_normal_steps(tmp_path_factory):
    off, on = c_run(tmp_path_factory, False), c_run(tmp_path_factory, True)
    # the overlapped branch ran: an update was still queued after each normal step
    assert all(q > 0 for q in on[0]["queued"][:2]) and not any(off[0]["queued"]), (on[0]["queued"], off[0]["queued"])
    for r in range(2):
        assert on[r]["norms"][:2] == off[r]["norms"][:2], (on[r]["norms"], off[r]["norms"])
        _same_state(on[r]["normal"], off[r]["normal"], "rank %d, two normal steps, overlap on against off" % r)
    _same_state(on[0]["normal"], on[1]["normal"], "replicas after two normal steps")


def test_overlapped_update_reduces_hand_written_gradients(tmp_path_factory):
    """in replicated mode a step over gradients no in-backward all-reduce
    finished must all-reduce them, with overlap_next_forward set as without."""
    off, on = c_run(tmp_path_factory, False), c_run(tmp_path_factory, True)
    for tag in ("hand", "after"):
        _same_state(off[0][tag], off[1][tag], "replicas, overlap off, %s" % tag)
        _same_state(on[0][tag], on[1][tag], "replicas, overlap on, %s" % tag)
        for r in range(2):
            _same_state(on[r][tag], off[r][tag], "rank %d, overlap on against off, %s" % (r, tag))
    assert on[0]["norms"] == on[1]["norms"] == off[0]["norms"] == off[1]["norms"]

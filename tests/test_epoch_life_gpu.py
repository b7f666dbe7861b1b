"""A scripted epoch through training_utils.train_one_epoch itself (tests/epoch_ref.py: the
scripts, the schedule, the gates; tests/test_epoch_ref.py proves them on the CPU and
shows eight mistakes of the kind looked for here breaking them).

What no other test composes: the overlapped update (FusedAdam.overlap_next_forward and
trust_backward_norm, as the loop sets them), an eval forward of another batch size right
after step() while that update is still queued, a smaller last batch (M changes inside
one engine, and with it the GEMM routes, the grouped cross k|v launch, the split-K
workspace, the workspace itself and the M-keyed fp8 buffers), and the epoch boundary
(scheduler step, state_dict reads, a checkpoint that is resumed from).

Run X  train_one_epoch once per epoch, scheduler.step() and save_checkpoint between
       epochs as train.train_model does, torch.manual_seed at the start of each epoch.
       print_training_progress and _validation_step are wrapped to record each step's
       (loss, norm) and each validation loss; the loop's own code runs.
Run Y  the same events one at a time, each on a fresh model and optimizer built from
       the state dicts the previous event left (no workspace, RoPE table, fp8 buffer,
       W^T copy or norm partial survives), overlap off, trust_backward_norm on (the
       norm path must be X's), torch's RNG state carried across each rebuild.

3a  X equals X, X equals Y and the epoch resumed from the checkpoint equals X's, bit for
    bit: every training loss, clip norm and validation loss, and after each epoch every
    parameter, both moments and the step count.  Both Adam kernels write the bf16 shadow
    with cast_kernel's rounding and the overlapped update is the in-order one per
    element, so equality is the expectation, not a tolerance.  The launch counters around
    single events of Y show that the full and the partial batch took different routes.
3b  Y against the float64 oracle, teacher-forced from Y's own state before the step
    (epoch_ref.teacher_forced_step): FP32 every training step of both epochs and every
    validation forward; BF16 the partial-batch step of epoch 0 and the first step of
    epoch 1 (new lr, nonzero moments, t = 5).  Gates: epoch_ref (the existing ones and
    the derived Adam bound).  FP8 has no oracle link (tests/test_fp8_gpu.py has its
    accuracy gates).
Figures of one MI355X run: profiles/epoch_life_errors.txt."""
import os
import shutil

import pytest
import torch

from tests import epoch_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["BF16", "FP32", "FP8"]


def components(name):
    from neurosync_trainer_lite_amd.utils.model_utils import build_model, prepare_training_components
    cfg = E.config(name)
    model = build_model(cfg, DEV)
    if E.SCRIPTS[name]["fp8"]:
        model.set_fp8(True, backward=True)
    crit, opt, sched = prepare_training_components(cfg, model)
    return cfg, model, crit, opt, sched


def by_name(model, opt):
    """(parameters, exp_avg, exp_avg_sq) as {state_dict key: CPU clone}."""
    named = dict(model.named_parameters())
    p = {k: v.detach().cpu().clone() for k, v in named.items()}
    m = {k: opt.state[v]["exp_avg"].detach().cpu().clone() for k, v in named.items()}
    v_ = {k: opt.state[v]["exp_avg_sq"].detach().cpu().clone() for k, v in named.items()}
    return p, m, v_


def end_state(model, opt):
    """What an epoch leaves: state_dict() syncs a queued update before anything is read."""
    sd = {k: v.cpu().clone() for k, v in model.state_dict().items()}
    osd = opt.state_dict()
    torch.cuda.synchronize()
    # the moments a checkpoint gets are the arenas' as they are now, at every epoch's end (a state_dict()
    # that detaches optimizer.state from the arenas keeps handing out those of its first call)
    eng = model.engine()
    for i, p in enumerate(opt.param_groups[0]["params"]):
        o, k, shp = eng.offsets[eng.name_of[id(p)]]
        for key, arena in (("exp_avg", opt.m), ("exp_avg_sq", opt.v)):
            assert torch.equal(osd["state"][i][key], arena[o:o + k].view(shp)), (i, key, eng.name_of[id(p)])
            assert opt.state[p][key]._base is arena, (i, key)
    return dict(sd=sd, osd=osd, m=opt.m.cpu().clone(), v=opt.v.cpu().clone(), step=opt._nstl_step,
                osd_steps=sorted({float(s["step"]) for s in osd["state"].values()}))


# ------------------------------------------------------------------------------- run X
def run_x(name, tmp, resume_from=None):
    """The real loop.  resume_from: (checkpoint path, first epoch to run): fresh model,
    optimizer and scheduler, load_checkpoint, then the remaining epochs.  Returns one
    record per epoch run and the path of the checkpoint written after each."""
    from neurosync_trainer_lite_amd.train import _NoScaler
    from neurosync_trainer_lite_amd.utils import checkpoint_utils, training_utils
    sc = E.SCRIPTS[name]
    train, val = E.batches(name)
    cfg, model, crit, opt, sched = components(name)
    eng = model.engine()
    first, batch_step = 0, 0
    if resume_from is None:
        model.load_state_dict(E.params(name), strict=True)
    else:
        path, first = resume_from
        epoch0, batch_step, model, opt, sched = checkpoint_utils.load_checkpoint(path, model, opt, sched, torch.device(DEV))
        assert epoch0 == first - 1 and batch_step == first * len(train)
    out, ckpts = [], []
    with pytest.MonkeyPatch.context() as mp:
        mp.chdir(tmp)  # the plots and the checkpoint land under tmp
        rec = {}
        real_val = training_utils._validation_step

        def progress(batch_idx, total_norm, batch_loss, batch_step, epoch, total_epochs, dataloader_len, pbar):
            assert opt.overlap_next_forward and opt.trust_backward_norm
            assert (batch_idx, dataloader_len, total_epochs) == (len(rec["steps"]), len(train), cfg["n_epochs"])
            rec["steps"].append((batch_loss, total_norm))
            rec["lrs"].append(opt.param_groups[0]["lr"])

        def validation(model_, val_iter, val_dl, criterion, device):
            assert opt.overlap_next_forward and opt.trust_backward_norm
            # the update of the step just taken is still queued: this forward consumes its stage waits
            queued = len(eng._wpending)
            r = real_val(model_, val_iter, val_dl, criterion, device)
            rec["vals"].append(r[1])
            rec["queued"].append((queued, len(eng._wpending)))
            assert model_.training
            return r

        mp.setattr(training_utils, "print_training_progress", progress)
        mp.setattr(training_utils, "_validation_step", validation)
        for epoch in range(first, sc["epochs"]):
            rec = dict(steps=[], vals=[], lrs=[], queued=[])
            torch.manual_seed(E.EPOCH_SEED + epoch)
            batch_step = training_utils.train_one_epoch(
                epoch, model, train, crit, opt, torch.device(DEV), clip=E.CLIP, batch_step=batch_step, pbar=None,
                total_epochs=cfg["n_epochs"], use_amp=cfg["use_amp"], grad_scaler=_NoScaler() if cfg["use_amp"] else None,
                val_dataloader=val, validation_interval=sc["interval"])
            assert not opt.overlap_next_forward and not opt.trust_backward_norm
            assert batch_step == (epoch + 1) * len(train)
            assert os.path.exists("dataset/validation_plots/loss/loss_epoch_%d.png" % (epoch + 1))
            rec.update(end_state(model, opt))
            sched.step()
            checkpoint_utils.save_checkpoint(model, opt, sched, epoch, batch_step, cfg)
            keep = os.path.join(str(tmp), "after_epoch_%d.pth" % epoch)
            shutil.copy(cfg["checkpoint_path"], keep)
            ckpts.append(keep)
            out.append(rec)
            if opt._overlap_allowed:
                # every validation forward started under a queued update and awaited all of it
                assert all(q > 0 and left == 0 for q, left in rec["queued"]), rec["queued"]
    return out, ckpts


# ------------------------------------------------------------------------------- run Y
def run_y(name, oracle_steps):
    """The same events, each on a fresh model and optimizer.  oracle_steps: the 1-based
    training steps whose state before, gradients, prediction and parameters after are
    kept for 3b (all validation forwards keep theirs when any step does)."""
    from neurosync_trainer_lite_amd import _hip as K
    sc = E.SCRIPTS[name]
    train, val = E.batches(name)
    model_sd, opt_sd = {k: v.clone() for k, v in E.params(name).items()}, None
    epochs, n = [], 0
    for epoch in range(sc["epochs"]):
        torch.manual_seed(E.EPOCH_SEED + epoch)
        rec = dict(steps=[], vals=[], events=[])
        for kind, i in E.events(name):
            rng = torch.get_rng_state()
            cfg, model, crit, opt, sched = components(name)
            model.load_state_dict(model_sd, strict=True)
            opt._bind()
            if opt_sd is not None:
                opt.load_state_dict(opt_sd)
            lr = E.lr_at(cfg, epoch)
            for g in opt.param_groups:
                g["lr"] = lr
            torch.set_rng_state(rng)
            eng = model.engine()
            opt.overlap_next_forward, opt.trust_backward_norm = False, True
            ev = dict(kind=kind, i=i, epoch=epoch)
            K.kernel_counts_reset()
            if kind == "train":
                n += 1
                src, trg = train[i]
                assert opt._nstl_step == n - 1
                model.train()
                opt.zero_grad()
                pred = model(src.to(DEV))
                loss = crit(pred, trg.to(DEV), current_step=n - 1, total_steps=cfg["n_epochs"] * len(train))
                loss.backward()
                torch.cuda.synchronize()
                ev.update(n=n, lr=lr, seed=eng.saved["seed"], counts=K.kernel_counts(), M=src.shape[0] * src.shape[1],
                          relu_bits_enc=list(eng.saved["bb"].e_rmask_ok), relu_bits_dec=list(eng.saved["bb"].d_rmask_ok),
                          kv_grouped=eng._kv_all_done, fused_norm=eng.sq_state is not None,
                          ws=eng.saved["bb"].ws.numel())
                assert eng.saved["p"] == sc["p"]
                if n in oracle_steps:
                    p, m, v = by_name(model, opt)
                    ev.update(before=dict(p=p, m=m, v=v), pred=pred.detach().cpu(),
                              grads={k: q.grad.detach().cpu().clone() for k, q in model.named_parameters()})
                opt.step(max_norm=E.CLIP)
                torch.cuda.synchronize()
                ev.update(loss=loss.item(), norm=opt.last_norm.item())
                if n in oracle_steps:
                    ev["params"] = by_name(model, opt)[0]
                rec["steps"].append((ev["loss"], ev["norm"]))
                model_sd, opt_sd = model.state_dict(), opt.state_dict()
            else:
                src, trg = val[i]
                model.eval()
                with torch.no_grad():
                    pred = model(src.to(DEV))
                    ev["loss"] = crit(pred, trg.to(DEV)).item()
                ev.update(n=n, counts=K.kernel_counts(), M=src.shape[0] * src.shape[1], T=src.shape[1])
                if oracle_steps:
                    ev.update(pred=pred.cpu(), params=by_name(model, opt)[0])
                rec["vals"].append(ev["loss"])
            rec["events"].append(ev)
        rec.update(end_state(model, opt))
        epochs.append(rec)
    return epochs


ORACLE_STEPS = {"BF16": (4, 5), "FP32": (1, 2, 3, 4, 5, 6), "FP8": ()}
_X, _Y, _R = {}, {}, {}


def x_of(name, k, tmp_path_factory):
    if (name, k) not in _X:
        _X[name, k] = run_x(name, tmp_path_factory.mktemp("x%d_%s" % (k, name)))
    return _X[name, k]


def y_of(name):
    if name not in _Y:
        _Y[name] = run_y(name, ORACLE_STEPS[name])
    return _Y[name]


def same_epoch(a, b, what):
    """Bit for bit: losses, norms, validation losses, parameters, moments, step count."""
    assert a["steps"] == b["steps"], (what, a["steps"], b["steps"])
    assert a["vals"] == b["vals"], (what, a["vals"], b["vals"])
    assert a["step"] == b["step"] and a["osd_steps"] == b["osd_steps"] == [float(a["step"])], (what, a["step"], b["step"])
    for k in a["sd"]:
        assert torch.equal(a["sd"][k], b["sd"][k]), (what, k, (a["sd"][k] - b["sd"][k]).abs().max().item())
    assert torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"]), what
    for i, s in a["osd"]["state"].items():
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(s[key], b["osd"]["state"][i][key]), (what, i, key)


def show_epochs(what, name, epochs, first=0):
    print("\n%s %s" % (what, name))
    for e, r in enumerate(epochs, first):
        print("  epoch %d  (loss, clip norm) %s" % (e, ["(%.9g, %.9g)" % s for s in r["steps"]]))
        print("           validation %s  step count %d" % (["%.9g" % v for v in r["vals"]], r["step"]))


# ---------------------------------------------------------------------------------- 3a
@pytest.mark.parametrize("name", NAMES)
def test_loop_is_reproducible_run_to_run(name, tmp_path_factory):
    (a, _), (b, _) = x_of(name, 0, tmp_path_factory), x_of(name, 1, tmp_path_factory)
    show_epochs("X", name, a)
    sc, cfg = E.SCRIPTS[name], E.config(name)
    assert len(a) == len(b) == sc["epochs"]
    for e, (ra, rb) in enumerate(zip(a, b)):
        assert len(ra["steps"]) == len(sc["train"]) and len(ra["vals"]) == sum(k == "val" for k, _ in E.events(name))
        assert all(v == v for s in ra["steps"] for v in s) and all(v == v for v in ra["vals"])  # no NaN
        assert ra["lrs"] == [E.lr_at(cfg, e)] * len(sc["train"]), ra["lrs"]
        assert ra["step"] == (e + 1) * len(sc["train"])
        same_epoch(ra, rb, "X run 0 against X run 1, epoch %d" % e)
    if sc["epochs"] > 1:
        assert a[0]["lrs"][0] != a[1]["lrs"][0]


@pytest.mark.parametrize("name", NAMES)
def test_loop_equals_the_same_events_one_at_a_time(name, tmp_path_factory):
    x, _ = x_of(name, 0, tmp_path_factory)
    y = y_of(name)
    show_epochs("Y", name, y)
    for e, (rx, ry) in enumerate(zip(x, y)):
        seeds = [ev["seed"] for ev in ry["events"] if ev["kind"] == "train"]
        assert seeds == E.epoch_seeds(e, len(seeds)), "one draw per training forward, none per eval forward"
        same_epoch(rx, ry, "X against Y, epoch %d" % e)


@pytest.mark.parametrize("name", ["BF16", "FP32"])
def test_epoch_resumed_from_the_checkpoint_equals_the_loop(name, tmp_path_factory):
    x, ckpts = x_of(name, 0, tmp_path_factory)
    r, _ = run_x(name, tmp_path_factory.mktemp("resume_" + name), resume_from=(ckpts[0], 1))
    show_epochs("resumed", name, r, first=1)
    assert len(r) == 1 and r[0]["lrs"] == x[1]["lrs"]
    same_epoch(x[1], r[0], "X's epoch 1 against the resumed epoch 1")
    # the checkpoint written after epoch 1 holds epoch 1's state (not the moments of an earlier state_dict())
    ck = torch.load(ckpts[1], map_location="cpu", weights_only=True)
    assert (ck["epoch"], ck["batch_step"]) == (1, x[1]["step"])
    for k, v in ck["model_state_dict"].items():
        assert torch.equal(v, x[1]["sd"][k]), k
    for i, s in ck["optimizer_state_dict"]["state"].items():
        assert float(s["step"]) == x[1]["step"]
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(s[key], x[1]["osd"]["state"][i][key].cpu()), (i, key)
    assert ck["optimizer_state_dict"]["param_groups"][0]["lr"] == E.lr_at(E.config(name), 2)


def launches(c):
    return {k: v for k, v in c.items() if v}


@pytest.mark.parametrize("name", NAMES)
def test_full_and_partial_batches_take_different_routes(name):
    sc = E.SCRIPTS[name]
    evs = [ev for r in y_of(name) for ev in r["events"]]
    print("\nroutes %s" % name)
    for ev in evs:
        extra = "" if ev["kind"] == "val" else "  relu bits enc %s dec %s  k|v grouped %s  fused norm %s  workspace %d" % (
            ev["relu_bits_enc"], ev["relu_bits_dec"], ev["kv_grouped"], ev["fused_norm"], ev["ws"])
        print("  e%d %-5s M %-5d %s%s" % (ev["epoch"], ev["kind"], ev["M"], launches(ev["counts"]), extra))
    steps = [ev for ev in evs if ev["kind"] == "train"]
    m_full = max(ev["M"] for ev in steps)
    full = [ev for ev in steps if ev["M"] == m_full]
    part = [ev for ev in steps if ev["M"] < m_full]
    assert full and part
    n_attn = 3 * sc["L"]
    if name == "FP32":
        # f32: every GEMM on the 128 kernel at both sizes; what changes with M is the split-K workspace
        for ev in steps:
            c = ev["counts"]
            assert c["gemm128"] > 0 and c["gemm4"] == c["gemm_ring"] == c["gemm_group"] == 0, launches(c)
            assert c["attn_fwd"] == n_attn and c["attn_bwd_split"] == n_attn and c["attn_fwd_generic"] == 0, launches(c)
        vals = [ev for ev in evs if ev["kind"] == "val"]
        for ev in vals:
            c = ev["counts"]
            if ev["T"] % 32:
                assert c["attn_fwd_generic"] == n_attn and c["attn_fwd"] == 0, (ev["T"], launches(c))
            else:
                assert c["attn_fwd"] == n_attn and c["attn_fwd_generic"] == 0, (ev["T"], launches(c))
        assert {ev["T"] for ev in vals} == {32, 40}
        return
    for ev in full:
        c = ev["counts"]
        # FFN1 is 32 tiles of 256^2: the 256-wide kernels, with the stored ReLU bits
        assert all(ev["relu_bits_enc"]) and all(ev["relu_bits_dec"]) and c["gemm_ring"] + c["gemm4"] > 0, launches(c)
        assert ev["fused_norm"]
        # the cross k|v projections of both layers in one grouped launch (bf16 projections only)
        assert ev["kv_grouped"] == (name == "BF16")
    for ev in part:
        c = ev["counts"]
        # 8 tiles: no side outputs from the bf16 FFN1 (the fp8 kernel, the encoder's FFN1 in FP8, stores them at any size)
        assert not any(ev["relu_bits_dec"]) and (name == "FP8" or not any(ev["relu_bits_enc"]))
        assert not ev["kv_grouped"] and c["gemm128"] > 0, launches(c)
    gemm = [k for k in full[0]["counts"] if k.startswith("gemm")]
    assert all([f["counts"][k] for k in gemm] != [p["counts"][k] for k in gemm] for f in full for p in part)
    assert all(f["ws"] > p["ws"] for f in full for p in part)  # the split-K count, and with it the workspace
    assert all(ev["counts"]["attn_fwd"] == n_attn and ev["counts"]["attn_bwd_fused"] == n_attn for ev in steps)


# ---------------------------------------------------------------------------------- 3b
def oracle_step(name, ev):
    sc, cfg = E.SCRIPTS[name], E.config(name)
    src, trg = E.batches(name)[0][ev["i"]]
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    b = ev["before"]
    ref = E.teacher_forced_step(b["p"], b["m"], b["v"], ev["n"] - 1, ev["lr"], src, trg,
                                E.masks_of(name, src.shape[0], src.shape[1], ev["seed"]), sc["H"], cfg["weight_decay"])
    return E.step_figures(ev, ref)


@pytest.mark.parametrize("n", ORACLE_STEPS["FP32"])
def test_fp32_steps_match_the_teacher_forced_oracle(n):
    ev = next(ev for r in y_of("FP32") for ev in r["events"] if ev["kind"] == "train" and ev["n"] == n)
    assert ev["lr"] == E.lr_at(E.config("FP32"), ev["epoch"])
    fig = oracle_step("FP32", ev)
    print("\n" + E.figure_line("FP32 step %d e%d b%d" % (n, ev["epoch"], ev["i"]), fig, ev["lr"], n))
    assert not E.broken_gates(fig, E.FP32_GATES, ev["lr"], n), fig


@pytest.mark.parametrize("n", ORACLE_STEPS["BF16"])
def test_bf16_steps_match_the_teacher_forced_oracle(n):
    ev = next(ev for r in y_of("BF16") for ev in r["events"] if ev["kind"] == "train" and ev["n"] == n)
    # the partial batch of epoch 0; the first step of epoch 1
    assert (ev["epoch"], ev["i"], ev["M"]) == {4: (0, 3, 384), 5: (1, 0, 2048)}[n]
    assert ev["lr"] == E.lr_at(E.config("BF16"), ev["epoch"])
    fig = oracle_step("BF16", ev)
    print("\n" + E.figure_line("BF16 step %d e%d b%d" % (n, ev["epoch"], ev["i"]), fig, ev["lr"], n))
    assert not E.broken_gates(fig, E.BF16_GATES, ev["lr"], n), fig


def test_fp32_validation_forwards_match_the_oracle():
    sc = E.SCRIPTS["FP32"]
    val = E.batches("FP32")[1]
    bad = []
    print()
    for r in y_of("FP32"):
        for ev in r["events"]:
            if ev["kind"] == "val":
                src, trg = val[ev["i"]]
                e_pred, e_loss = E.val_figures(ev["params"], src, trg, sc["H"], ev["pred"], ev["loss"])
                print("FP32 val after step %d e%d v%d T%d   pred %.2e loss %.2e" % (ev["n"], ev["epoch"], ev["i"], ev["T"],
                                                                                   e_pred, e_loss))
                if not (e_pred < E.VAL_GATE and e_loss < E.VAL_GATE):
                    bad.append((ev["n"], ev["i"], e_pred, e_loss))
    assert not bad, bad

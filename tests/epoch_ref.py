"""TEST INFRA: a scripted epoch and the references that judge it, with no GPU dependency.
tests/test_epoch_ref.py proves what is here on the CPU (the Adam bound, teacher forcing,
eight mutants); tests/test_epoch_life_gpu.py drives training_utils.train_one_epoch through
the scripts and judges every event by it.  Never imported by the package.

The script.  An epoch is a plain list of (src, trg) CPU tensors (train_one_epoch needs
only len and iter), a training list and a validation list, seeded with numpy's
default_rng (inputs as test_dropout_step_parity_gpu.batch).  The last training batch
is smaller, as with a loader that has no drop_last, so M changes inside one engine:

  BF16  D256 H4 L2 p 0.1, bf16    train [B16, B16, B16, B3] T128   val [B16 T128, B3 T128]
        every 2 batches, 2 epochs.  B16 T128 is 2048 rows (FFN1 32 tiles of 256^2: the
        GEMMs that store the ReLU bits, the grouped cross k|v launch); B3 T128 is 384.
  FP32  D128 H2 L2 p 0.1, f32     train [B4, B4, B3] T32           val [B2 T32, B2 T40]
        every 2 batches, 2 epochs.  T40 is ragged: generic attention there.
  FP8   the BF16 model with set_fp8(True, backward=True)
                                  train [B16, B3, B16] T128        val [B3 T128]
        every batch, 1 epoch: every event replaces the M-keyed fp8 buffers.

Schedule: warmup_epochs 0 and n_epochs 2, so prepare_training_components' LambdaLR gives
the factor 1 in epoch 0 and 1/2 in epoch 1 (model_ref.lr_lambda).

Gates of a training step judged against the float64 oracle started from the run's own
state before that step (teacher forcing): those of tests/test_dropout_step_parity_gpu.py
for the loss, the prediction, the clip norm and every gradient, and for the parameters
after step t the derived bound 2 x adam_ratio_bound(t) x lr per element (plus one f32
ulp of the parameter as stored) and lr / 2 on a tensor's mean."""
import math

import numpy as np
import torch

from neurosync_trainer_lite_amd.config import training_config
from oracle import model_ref
from tests import step_ref as S

IN_DIM, OUT_DIM = 256, 61
PARAM_SEED = 41
DATA_SEED = 300
EPOCH_SEED = 70  # torch.manual_seed(EPOCH_SEED + epoch) at the start of each epoch
CLIP = 2.0

SCRIPTS = {
    "BF16": dict(D=256, H=4, L=2, p=0.1, amp=True, fp8=False, train=[(16, 128)] * 3 + [(3, 128)],
                 val=[(16, 128), (3, 128)], interval=2, epochs=2),
    "FP32": dict(D=128, H=2, L=2, p=0.1, amp=False, fp8=False, train=[(4, 32), (4, 32), (3, 32)],
                 val=[(2, 32), (2, 40)], interval=2, epochs=2),
    "FP8": dict(D=256, H=4, L=2, p=0.1, amp=True, fp8=True, train=[(16, 128), (3, 128), (16, 128)],
                val=[(3, 128)], interval=1, epochs=1),
}

# pred: numpy.allclose with rtol = atol (fp32) or ||a - b|| / ||b|| (bf16)
FP32_GATES = {"grad": 1e-4, "pred": 1e-4, "loss": 1e-5, "norm": 1e-4, "pred_allclose": True}
BF16_GATES = {"grad": 0.1, "pred": 3e-2, "loss": 2e-2, "norm": 0.1, "pred_allclose": False}
VAL_GATE = 1e-4


def config(name):
    sc = SCRIPTS[name]
    cfg = dict(training_config)
    cfg.update(hidden_dim=sc["D"], num_heads=sc["H"], n_layers=sc["L"], dropout=sc["p"], use_amp=sc["amp"],
               warmup_epochs=0, n_epochs=2, checkpoint_path="out/checkpoints/checkpoint.pth")
    return cfg


def params(name):
    sc = SCRIPTS[name]
    return model_ref.seeded_params(model_ref.param_shapes(IN_DIM, sc["D"], sc["L"], OUT_DIM), PARAM_SEED)


def lr_at(cfg, epoch):
    """The learning rate LambdaLR leaves in the optimizer during `epoch`."""
    return cfg["learning_rate"] * model_ref.lr_lambda(epoch, cfg["warmup_epochs"], cfg["n_epochs"])


def batches(name):
    """(training list, validation list) of (src, trg) float32 CPU tensors."""
    sc = SCRIPTS[name]
    rng = np.random.default_rng(DATA_SEED)

    def one(B, T):
        src = torch.tensor(rng.standard_normal((B, T, IN_DIM)).astype(np.float32))
        trg = torch.tensor((rng.standard_normal((B, T, OUT_DIM)) * 20).astype(np.float32))
        return src, trg
    return [one(*bt) for bt in sc["train"]], [one(*bt) for bt in sc["val"]]


def events(name):
    """One epoch as train_one_epoch runs it: [("train", i) | ("val", j)]; a validation
    forward after batch i when i % validation_interval == 0, the validation list read in
    order from its start in every epoch and wrapping round."""
    sc = SCRIPTS[name]
    out, j = [], 0
    for i in range(len(sc["train"])):
        out.append(("train", i))
        if i % sc["interval"] == 0:
            out.append(("val", j % len(sc["val"])))
            j += 1
    return out


def epoch_seeds(epoch, n, seed_salt=0):
    """The base seeds of the n training forwards of `epoch`: one torch.randint draw each
    after torch.manual_seed(EPOCH_SEED + epoch), none for an eval forward.  Leaves torch's
    RNG state as it found it."""
    state = torch.get_rng_state()
    torch.manual_seed(EPOCH_SEED + epoch)
    out = [S.salted_seed(int(torch.randint(0, 2 ** 62, (1,)).item()), seed_salt) for _ in range(n)]
    torch.set_rng_state(state)
    return out


def masks_of(name, B, T, seed):
    sc = SCRIPTS[name]
    return S.site_masks(seed, B, T, sc["D"], sc["H"], sc["L"], sc["p"])


# ------------------------------------------------------------------------- the bound
def adam_ratio_bound(t, b1=0.9, b2=0.999):
    """The largest |m_hat_t| / sqrt(v_hat_t) over all gradient sequences g_1..g_t.
    m_t = (1 - b1) sum_j b1^j g_{t-j}, v_t = (1 - b2) sum_j b2^j g_{t-j}^2 (j < t), so by
    Cauchy-Schwarz on (b1^j / b2^(j/2)) (b2^(j/2) g_{t-j})
        |m_t| <= (1 - b1) sqrt(S_t) sqrt(v_t / (1 - b2)),   S_t = sum_{j<t} (b1^2 / b2)^j,
    with equality for g_{t-j} ~ (b1 / b2)^j, and with the bias corrections
        |m_hat| / sqrt(v_hat) <= (1 - b1) / (1 - b1^t) sqrt(S_t) sqrt((1 - b2^t) / (1 - b2)).
    eps > 0 only lowers the ratio.  1 at t = 1, 1.0013 at t = 2."""
    s = sum((b1 * b1 / b2) ** j for j in range(t))
    return (1 - b1) / (1 - b1 ** t) * math.sqrt(s) * math.sqrt((1 - b2 ** t) / (1 - b2))


def extremal_sequence(t, b1=0.9, b2=0.999):
    """g_1..g_t attaining adam_ratio_bound(t)."""
    return [(b1 / b2) ** (t - 1 - i) for i in range(t)]


def adam_ratio(g, b1=0.9, b2=0.999):
    """m_hat / sqrt(v_hat) after the last gradient of each row of g [n, t] (eps = 0;
    an all-zero row gives 0)."""
    g = np.asarray(g, dtype=np.float64)
    m, v = np.zeros(g.shape[0]), np.zeros(g.shape[0])
    t = g.shape[1]
    for i in range(t):
        m = b1 * m + (1 - b1) * g[:, i]
        v = b2 * v + (1 - b2) * g[:, i] ** 2
    den = np.sqrt(v / (1 - b2 ** t))
    return np.divide(m / (1 - b1 ** t), den, out=np.zeros_like(m), where=den > 0)


# -------------------------------------------------------------------- teacher forcing
def teacher_forced_step(params, m, v, step, lr, src, trg, masks, num_heads, wd, clip=CLIP):
    """One float64 oracle step from a given state: parameters, moments ({key: tensor}),
    `step` steps already taken, learning rate `lr`; masks from step_ref.site_masks with
    that step's base seed (None: no dropout).  Nothing of the caller's is modified."""
    o = model_ref.OracleTrainer(params, num_heads, lr=lr, weight_decay=wd, clip=clip, dtype=torch.float64)
    o.m = [m[k].detach().to("cpu", torch.float64).clone() for k in o.keys]
    o.v = [v[k].detach().to("cpu", torch.float64).clone() for k in o.keys]
    o.step_count = int(step)
    loss, norm, pred = o.step(src.double(), trg.double(), masks=masks)
    return dict(loss=loss.item(), pred=pred, norm=norm.item(), grads=o.last_grads,
                params={k: o.p[k].detach() for k in o.keys}, m=dict(zip(o.keys, o.m)), v=dict(zip(o.keys, o.v)),
                step=o.step_count)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def step_figures(run, ref):
    """Errors of one training step of the code under test (`run`: loss, norm floats;
    pred, grads {key}, params {key} after the step) against teacher_forced_step's `ref`."""
    grads = {k: rel(run["grads"][k], ref["grads"][k]) for k in ref["grads"]}
    worst = max(grads, key=grads.get)
    a, b = run["pred"].detach().double().cpu(), ref["pred"].double()
    diff = {k: (run["params"][k].detach().double().cpu() - ref["params"][k]).abs() for k in ref["params"]}
    return {
        "loss": abs(run["loss"] - ref["loss"]) / abs(ref["loss"]),
        "norm": abs(run["norm"] - ref["norm"]) / ref["norm"],
        "pred": rel(a, b),
        # numpy.allclose(a, b, rtol = atol = x) holds exactly when x >= this
        "pred_close": ((a - b).abs() / (1 + b.abs())).max().item(),
        "grad": grads[worst], "grad_at": worst,
        # worst element past the f32 storage rounding of the parameter; worst tensor mean
        "step_err": max((diff[k].max() - 2.0 ** -23 * ref["params"][k].abs().max()).item() for k in diff),
        "mean_step": max(d.mean().item() for d in diff.values()),
    }


def broken_gates(fig, gates, lr, t):
    """Names of the gates the figures of step t (1-based count of this step) break."""
    bad = []
    if not fig["grad"] < gates["grad"]:
        bad.append("grad")
    if not (fig["pred_close"] <= gates["pred"] if gates["pred_allclose"] else fig["pred"] < gates["pred"]):
        bad.append("pred")
    if not fig["loss"] < gates["loss"]:
        bad.append("loss")
    if not fig["norm"] < gates["norm"]:
        bad.append("norm")
    if not fig["step_err"] <= 2 * adam_ratio_bound(t) * lr:
        bad.append("param")
    if not fig["mean_step"] <= 0.5 * lr:
        bad.append("param_mean")
    return bad


def figure_line(tag, fig, lr, t):
    return ("%-28s loss %.2e pred %.2e close %.2e norm %.2e grad %.2e step %.3f mean %.3f (x lr %.2e, t %d, bound %.4f)  %s"
            % (tag, fig["loss"], fig["pred"], fig["pred_close"], fig["norm"], fig["grad"], fig["step_err"] / lr,
               fig["mean_step"] / lr, lr, t, adam_ratio_bound(t), fig["grad_at"]))


def val_figures(params, src, trg, num_heads, pred, loss):
    """An eval forward of the code under test against seq2seq_forward in float64 on the
    same parameters: (rel of the prediction, relative error of the loss)."""
    p64 = {k: v.detach().to("cpu", torch.float64) for k, v in params.items()}
    with torch.no_grad():
        want = model_ref.seq2seq_forward(p64, src.double(), num_heads)
        want_loss = model_ref.loss_fn(want, trg.double()).item()
    return rel(pred, want), abs(loss - want_loss) / abs(want_loss)

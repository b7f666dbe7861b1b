"""The kernels a call launches are the ones its route names: for the rows of
tests/test_attn_route_cpu.py's table with T <= 300, one nstl_attn_fwd and one nstl_attn_bwd
(B = 1, H = 2, p = 0.3 with stored keep bits, side buffers sized by the two queries) move
exactly the launch counter of the family in nstl_attn_route_describe's text, and every
output is finite.  Nothing numeric beyond that: the parity files own the numbers."""
import pytest
import torch

from tests.test_attn_route_cpu import BF16, MODES, TABLE

pytestmark = pytest.mark.gpu

B, H, P_DROP = 1, 2, 0.3
SWITCHES = ("NSTL_ATTN_LONG", "NSTL_ATTN_RAGGED", "NSTL_ATTN_FWD", "NSTL_ATTN_BWD", "NSTL_ROPE_BWD")
STORED = MODES[2][3]     # the slots of "p = 0.3, stored keep bits"
FWD_COUNTER = {"generic": "attn_fwd_generic", "one-shot": "attn_fwd", "streaming": "attn_fwd_long"}
BWD_COUNTER = {"generic": "attn_bwd_generic", "fused": "attn_bwd_fused", "split": "attn_bwd_split",
               "streaming": "attn_bwd_long"}
ROWS = [r for r in TABLE if r[1]["T"] <= 300]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_the_family_the_route_names_is_the_one_that_runs(row, monkeypatch):
    from neurosync_trainer_lite_amd import _hip as K
    name, kw, env, fwd_text, bwd_text, _, _ = row
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s, v in env.items():
        monkeypatch.setenv(s, v)
    T, dh, flags = kw["T"], kw.get("dh", 64), kw.get("flags", 7)
    dt = torch.bfloat16 if kw.get("dtype", BF16) == BF16 else torch.float32
    g = torch.Generator(device="cuda").manual_seed(1234)
    q, k, v, do = (torch.randn(B * T, H * dh, device="cuda", generator=g).to(dt) for _ in range(4))
    o, dq, dk, dv = (torch.full((B * T, H * dh), float("nan"), device="cuda", dtype=dt) for _ in range(4))
    lse, dsum = (torch.full((B * H * T,), float("nan"), device="cuda") for _ in range(2))
    a = K.attn_args(K.dtype_code(dt), B, T, H, 0, 0, 0, 0, 0, 0, 0, 0, 0, P_DROP, 99, dh=dh, flags=flags)
    words, rows = K.attn_mask_words(a), K.attn_bias_rows(a)
    mask = torch.zeros(words or (B * H * T * T + 63) // 64, dtype=torch.int64, device="cuda")
    part = torch.full((rows, 3 * H * dh), float("nan"), device="cuda") if rows else None
    K.attn_set(a, q=q, k=k, v=v, o=o, lse=lse, dout=do, dq=dq, dk=dk, dv=dv, dsum=dsum, mask_bits=mask, dbias_part=part)
    fwd, bwd = K.attn_route(a), K.attn_route(a, backward=True)
    assert (fwd, bwd) == (fwd_text.format(**STORED), bwd_text.format(**STORED))
    fwd_family, bwd_family = fwd.split()[0], bwd.split()[0]
    if bwd_family == "one-shot":
        bwd_family = bwd.split()[2]     # "one-shot bwd fused ..." / "one-shot bwd split ..."
    want = dict.fromkeys(K.KERNEL_COUNT_NAMES, 0)
    want[FWD_COUNTER[fwd_family]] = want[BWD_COUNTER[bwd_family]] = 1
    K.kernel_counts_reset()
    K.attn_fwd(a)
    K.attn_bwd(a)
    torch.cuda.synchronize()
    assert K.kernel_counts() == want, (name, fwd, bwd)
    for nm, t in dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, dbias_part=part).items():
        assert t is None or torch.isfinite(t.float()).all(), "%s: %s is not finite (%s / %s)" % (name, nm, fwd, bwd)

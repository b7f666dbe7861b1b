"""The attention routing as the host sees it, without a GPU: what nstl_attn_route_describe
and the two size queries (nstl_attn_mask_words, nstl_attn_bias_rows) answer over a literal
table of argument sets and switches.  The expected texts are written from the rule in
include/nstl.h (the table above nstl_attn_args) and the wording documented next to
nstl_attn_route_describe, not from the library's output.  All of it is host arithmetic,
so the pointers are fake (16-byte aligned integers) and nothing is launched.

Like tests/test_abi.py, every check runs in a child process: the library is never loaded
into the pytest process.

What only this table sees: a call routed to the `hi` kernels at head_dim 32, or to the
ragged form at head_dim 64 and T % 32 == 0, computes the right numbers, only slower; no
parity test notices."""
import json

from tests.test_abi import run_child

F32, BF16 = 0, 1
R, W, A = 1, 2, 4           # NSTL_ATTN_RAGGED_OK, _DH128_OK, _DHANY_OK
ALL = R | W | A
B, H = 2, 3                 # CHILD's mk(): words = 24 * ceil(T / 16)^2, rows = 2 * ceil(T / 128)

# every row runs under each: (name, p_drop, mask_bits set), and what the texts' slots then hold
MODES = [
    ("p = 0", 0.0, False, dict(drop=0, dm=0, mask="")),
    ("p = 0.3, hashed", 0.3, False, dict(drop=1, dm=2, mask="")),
    ("p = 0.3, stored keep bits", 0.3, True, dict(drop=1, dm=1, mask=" mask")),
]

GEN, GEN32 = "generic bf16", "generic f32"
FUSED0 = "one-shot bwd fused TC=0 dm={dm} rope_fast=1"
FUSED128 = "one-shot bwd fused TC=128 dm={dm} rope_fast=1"
SPLIT = "one-shot bwd split bf16 dm={dm} rope_fast=1"
PERSIST = "one-shot fwd persistent{mask}"
S_FWD = "streaming fwd DHT=%s drop={drop}"               # % "64", "64 rag", "128 any lo rag", ...
S_BWD = "streaming bwd DHT=%s dm={dm} rope_fast=1"

# (name, arguments over mk()'s defaults: bf16, dh 64, every flag), switches, forward text, backward text, words, rows)
TABLE = [
    # --- one-shot, bf16, head_dim 64
    ("T 32", dict(T=32), {}, "one-shot fwd bf16 NKT=2", FUSED0, 96, 2),
    ("T 32, flags 0", dict(T=32, flags=0), {}, "one-shot fwd bf16 NKT=2", FUSED0, 96, 2),
    ("T 96", dict(T=96), {}, "one-shot fwd bf16 NKT=6", FUSED0, 864, 2),
    ("T 128", dict(T=128), {}, PERSIST, FUSED128, 1536, 2),
    ("T 128, flags 0", dict(T=128, flags=0), {}, PERSIST, FUSED128, 1536, 2),
    ("T 128, NSTL_ATTN_FWD=oneshot", dict(T=128), {"NSTL_ATTN_FWD": "oneshot"}, "one-shot fwd bf16 NKT=8", FUSED128, 1536, 2),
    ("T 128, NSTL_ATTN_BWD=split", dict(T=128), {"NSTL_ATTN_BWD": "split"}, PERSIST, SPLIT, 1536, 2),
    ("T 96, NSTL_ATTN_BWD=split", dict(T=96), {"NSTL_ATTN_BWD": "split"}, "one-shot fwd bf16 NKT=6", SPLIT, 864, 2),
    ("T 160", dict(T=160), {}, "one-shot fwd bf16 NKT=10", SPLIT, 2400, 4),
    ("T 256", dict(T=256), {}, "one-shot fwd bf16 NKT=16", SPLIT, 6144, 4),
    ("T 128, NSTL_ROPE_BWD=table", dict(T=128), {"NSTL_ROPE_BWD": "table"}, PERSIST,
     "one-shot bwd fused TC=128 dm={dm} rope_fast=0", 1536, 2),
    ("T 256, NSTL_ROPE_BWD=table", dict(T=256), {"NSTL_ROPE_BWD": "table"}, "one-shot fwd bf16 NKT=16",
     "one-shot bwd split bf16 dm={dm} rope_fast=0", 6144, 4),
    ("T 128, NSTL_ATTN_LONG=0", dict(T=128), {"NSTL_ATTN_LONG": "0"}, PERSIST, FUSED128, 1536, 2),
    ("T 128, NSTL_ATTN_RAGGED=0", dict(T=128), {"NSTL_ATTN_RAGGED": "0"}, PERSIST, FUSED128, 1536, 2),
    # --- f32, head_dim 64
    ("f32 T 32", dict(dtype=F32, T=32), {}, "one-shot fwd f32 NKT=2", "one-shot bwd split f32 dm={dm} rope_fast=1", 96, 2),
    ("f32 T 128", dict(dtype=F32, T=128), {}, "one-shot fwd f32 NKT=8", "one-shot bwd split f32 dm={dm} rope_fast=1", 1536, 2),
    ("f32 T 160", dict(dtype=F32, T=160), {}, GEN32, GEN32, 0, 0),
    ("f32 T 100", dict(dtype=F32, T=100), {}, GEN32, GEN32, 0, 0),
    ("f32 T 288", dict(dtype=F32, T=288), {}, GEN32, GEN32, 0, 0),
    # --- streaming, head_dim 64
    ("T 288, flags 0", dict(T=288, flags=0), {}, S_FWD % "64", S_BWD % "64", 7776, 6),
    ("T 288", dict(T=288), {}, S_FWD % "64", S_BWD % "64", 7776, 6),
    ("T 4096", dict(T=4096), {}, S_FWD % "64", S_BWD % "64", 1572864, 64),
    ("T 300, RAGGED_OK", dict(T=300, flags=R), {}, S_FWD % "64 rag", S_BWD % "64 rag", 8664, 6),
    ("T 300, flags 0", dict(T=300, flags=0), {}, GEN, GEN, 0, 0),
    ("T 300, DH128_OK | DHANY_OK", dict(T=300, flags=W | A), {}, GEN, GEN, 0, 0),
    ("T 100, RAGGED_OK", dict(T=100, flags=R), {}, S_FWD % "64 rag", S_BWD % "64 rag", 1176, 2),
    ("T 7, RAGGED_OK", dict(T=7, flags=R), {}, S_FWD % "64 rag", S_BWD % "64 rag", 24, 2),
    ("T 4095, RAGGED_OK", dict(T=4095, flags=R), {}, S_FWD % "64 rag", S_BWD % "64 rag", 1572864, 64),
    ("T 100, flags 0", dict(T=100, flags=0), {}, GEN, GEN, 0, 0),
    ("T 300, RAGGED_OK, NSTL_ATTN_RAGGED=0", dict(T=300, flags=R), {"NSTL_ATTN_RAGGED": "0"}, GEN, GEN, 0, 0),
    ("T 288, NSTL_ATTN_RAGGED=0", dict(T=288), {"NSTL_ATTN_RAGGED": "0"}, S_FWD % "64", S_BWD % "64", 7776, 6),
    ("T 288, NSTL_ATTN_LONG=0", dict(T=288), {"NSTL_ATTN_LONG": "0"}, GEN, GEN, 0, 0),
    ("T 300, NSTL_ATTN_LONG=0", dict(T=300), {"NSTL_ATTN_LONG": "0"}, GEN, GEN, 0, 0),
    ("T 288, NSTL_ROPE_BWD=table", dict(T=288), {"NSTL_ROPE_BWD": "table"}, S_FWD % "64",
     "streaming bwd DHT=64 dm={dm} rope_fast=0", 7776, 6),
    ("T 288, the one-shot switches", dict(T=288), {"NSTL_ATTN_FWD": "oneshot", "NSTL_ATTN_BWD": "split"},
     S_FWD % "64", S_BWD % "64", 7776, 6),
    # --- streaming, head_dim 128
    ("dh 128 T 32, DH128_OK", dict(dh=128, T=32, flags=W), {}, S_FWD % "128", S_BWD % "128", 96, 2),
    ("dh 128 T 128, DH128_OK", dict(dh=128, T=128, flags=W), {}, S_FWD % "128", S_BWD % "128", 1536, 2),
    ("dh 128 T 288, every flag", dict(dh=128, T=288), {}, S_FWD % "128", S_BWD % "128", 7776, 6),
    ("dh 128 T 32, DHANY_OK only", dict(dh=128, T=32, flags=A), {}, GEN, GEN, 0, 0),
    ("dh 128 T 32, flags 0", dict(dh=128, T=32, flags=0), {}, GEN, GEN, 0, 0),
    ("dh 128 T 7, DH128_OK only", dict(dh=128, T=7, flags=W), {}, GEN, GEN, 0, 0),
    ("dh 128 T 7, DH128_OK | RAGGED_OK", dict(dh=128, T=7, flags=W | R), {}, S_FWD % "128 rag", S_BWD % "128 rag", 24, 2),
    ("dh 128 T 300, DH128_OK | RAGGED_OK", dict(dh=128, T=300, flags=W | R), {}, S_FWD % "128 rag", S_BWD % "128 rag", 8664, 6),
    ("dh 128 T 32, NSTL_ATTN_LONG=0", dict(dh=128, T=32), {"NSTL_ATTN_LONG": "0"}, GEN, GEN, 0, 0),
    ("dh 128 f32 T 32", dict(dtype=F32, dh=128, T=32), {}, GEN32, GEN32, 0, 0),
    # --- streaming, the other widths: the runtime-width kernels, always the ragged form
    ("dh 8 T 32", dict(dh=8, T=32, flags=A), {}, S_FWD % "64 any lo rag", S_BWD % "64 any lo rag", 96, 2),
    ("dh 8 T 288", dict(dh=8, T=288, flags=A), {}, S_FWD % "64 any lo rag", S_BWD % "64 any lo rag", 7776, 6),
    ("dh 32 T 32", dict(dh=32, T=32, flags=A), {}, S_FWD % "64 any lo rag", S_BWD % "64 any lo rag", 96, 2),
    ("dh 32 T 288", dict(dh=32, T=288, flags=A), {}, S_FWD % "64 any lo rag", S_BWD % "64 any lo rag", 7776, 6),
    ("dh 40 T 32", dict(dh=40, T=32, flags=A), {}, S_FWD % "64 any hi rag", S_BWD % "64 any hi rag", 96, 2),
    ("dh 40 T 288", dict(dh=40, T=288, flags=A), {}, S_FWD % "64 any hi rag", S_BWD % "64 any hi rag", 7776, 6),
    ("dh 56 T 32", dict(dh=56, T=32, flags=A), {}, S_FWD % "64 any hi rag", S_BWD % "64 any hi rag", 96, 2),
    ("dh 56 T 288", dict(dh=56, T=288, flags=A), {}, S_FWD % "64 any hi rag", S_BWD % "64 any hi rag", 7776, 6),
    ("dh 72 T 32", dict(dh=72, T=32, flags=A), {}, S_FWD % "128 any lo rag", S_BWD % "128 any lo rag", 96, 2),
    ("dh 72 T 288", dict(dh=72, T=288, flags=A), {}, S_FWD % "128 any lo rag", S_BWD % "128 any lo rag", 7776, 6),
    ("dh 96 T 32", dict(dh=96, T=32, flags=A), {}, S_FWD % "128 any lo rag", S_BWD % "128 any lo rag", 96, 2),
    ("dh 96 T 288", dict(dh=96, T=288, flags=A), {}, S_FWD % "128 any lo rag", S_BWD % "128 any lo rag", 7776, 6),
    ("dh 104 T 32", dict(dh=104, T=32, flags=A), {}, S_FWD % "128 any hi rag", S_BWD % "128 any hi rag", 96, 2),
    ("dh 104 T 288", dict(dh=104, T=288, flags=A), {}, S_FWD % "128 any hi rag", S_BWD % "128 any hi rag", 7776, 6),
    ("dh 120 T 32", dict(dh=120, T=32, flags=A), {}, S_FWD % "128 any hi rag", S_BWD % "128 any hi rag", 96, 2),
    ("dh 120 T 288", dict(dh=120, T=288, flags=A), {}, S_FWD % "128 any hi rag", S_BWD % "128 any hi rag", 7776, 6),
    ("dh 120 T 300, DHANY_OK | RAGGED_OK", dict(dh=120, T=300, flags=A | R), {},
     S_FWD % "128 any hi rag", S_BWD % "128 any hi rag", 8664, 6),
    ("dh 56 T 7, DHANY_OK | RAGGED_OK", dict(dh=56, T=7, flags=A | R), {}, S_FWD % "64 any hi rag", S_BWD % "64 any hi rag", 24, 2),
    ("dh 56 T 7, DHANY_OK only", dict(dh=56, T=7, flags=A), {}, GEN, GEN, 0, 0),
    ("dh 56 T 7, NSTL_ATTN_RAGGED=0", dict(dh=56, T=7), {"NSTL_ATTN_RAGGED": "0"}, GEN, GEN, 0, 0),
    ("dh 56 T 288, NSTL_ATTN_RAGGED=0", dict(dh=56, T=288), {"NSTL_ATTN_RAGGED": "0"},
     S_FWD % "64 any hi rag", S_BWD % "64 any hi rag", 7776, 6),
    ("dh 56 T 32, NSTL_ATTN_LONG=0", dict(dh=56, T=32), {"NSTL_ATTN_LONG": "0"}, GEN, GEN, 0, 0),
    ("dh 32 T 32, DH128_OK | RAGGED_OK", dict(dh=32, T=32, flags=W | R), {}, GEN, GEN, 0, 0),
    ("dh 32 T 32, flags 0", dict(dh=32, T=32, flags=0), {}, GEN, GEN, 0, 0),
    ("dh 32 f32 T 32", dict(dtype=F32, dh=32, T=32), {}, GEN32, GEN32, 0, 0),
] + [
    # --- generic by width, whatever the flags
    ("dh %d T %d" % (dh, T), dict(dh=dh, T=T), {}, GEN, GEN, 0, 0)
    for dh in (136, 256, 512) for T in (7, 32, 128, 288, 300, 4096)
]

# arguments nstl_attn_fwd / nstl_attn_bwd reject for their shape: (name, arguments, text)
REJECTED = [
    ("dh 4", dict(dh=4, T=32), "rejected: nstl_attn: head_dim must be a multiple of 8 up to 512 (got 4)"),
    ("dh 12", dict(dh=12, T=32), "rejected: nstl_attn: head_dim must be a multiple of 8 up to 512 (got 12)"),
    ("dh 520", dict(dh=520, T=32), "rejected: nstl_attn: head_dim must be a multiple of 8 up to 512 (got 520)"),
    ("T 0", dict(T=0), "rejected: nstl_attn: T must be in [1, 4096] (got 0)"),
    ("T 4097", dict(T=4097), "rejected: nstl_attn: T must be in [1, 4096] (got 4097)"),
    ("dtype 7", dict(dtype=7, T=32), "rejected: nstl_attn: bad dtype"),
    ("B 0", dict(B=0, T=32), "rejected: nstl_attn: empty batch"),
    ("H 0", dict(H=0, T=32), "rejected: nstl_attn: empty batch"),
    ("p_drop 1.0", dict(p_drop=1.0, T=32), "rejected: nstl_attn: p_drop out of range"),
    ("p_drop -0.1", dict(p_drop=-0.1, T=288), "rejected: nstl_attn: p_drop out of range"),
]

CHILD = """
    import ctypes, json, os
    from neurosync_trainer_lite_amd import _hip
    lib = _hip.lib()
    SWITCHES = ("NSTL_ATTN_LONG", "NSTL_ATTN_RAGGED", "NSTL_ATTN_FWD", "NSTL_ATTN_BWD", "NSTL_ROPE_BWD")

    def mk(dtype=1, B=2, H=3, T=128, dh=64, flags=7, p_drop=0.0, mask=False):
        ld = H * dh
        a = _hip.attn_args(dtype, B, T, H, 0x1000, ld, 0x2000, ld, 0x3000, ld, 0x4000, ld, 0x5000, p_drop, 7, dh=dh, flags=flags)
        a.dout, a.dq, a.dk, a.dv = 0x6000, 0x7000, 0x8000, 0x9000
        a.dout_ld = a.dq_ld = a.dk_ld = a.dv_ld = ld
        a.dsum = 0xa000
        a.mask_bits = 0xb000 if mask else None
        return a

    def answers(kw, env, p_drop, mask):
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        kw = dict(dict(p_drop=p_drop), **kw)
        a = mk(mask=mask, **kw)
        return [_hip.attn_route(a), _hip.attn_route(a, backward=True), _hip.attn_mask_words(a), _hip.attn_bias_rows(a)]
"""


def test_route_and_sizes_over_the_table():
    out = run_child(CHILD + """
    rows, modes = json.loads(sys.argv[1]), json.loads(sys.argv[2])
    print(json.dumps([[answers(kw, env, p, m) for p, m in modes] for kw, env in rows]))
    """, json.dumps([(kw, env) for _, kw, env, _, _, _, _ in TABLE]), json.dumps([(p, m) for _, p, m, _ in MODES]))
    got = json.loads(out.strip().splitlines()[-1])
    assert len(got) == len(TABLE)
    bad = []
    for (name, _, _, fwd, bwd, words, rows), per_mode in zip(TABLE, got):
        for (mode, _, _, slots), g in zip(MODES, per_mode):
            want = [fwd.format(**slots), bwd.format(**slots), words, rows]
            if g != want:
                bad.append("%s, %s: %s, expected %s" % (name, mode, g, want))
    assert not bad, "\n".join(bad)


def test_rejected_shapes_answer_zero_and_launch_nothing():
    out = run_child(CHILD + """
    _hip.kernel_counts_reset()
    got = []
    for kw in json.loads(sys.argv[1]):
        for p, m in json.loads(sys.argv[2]):
            kw2 = dict(dict(p_drop=p), **kw)
            a = mk(mask=m, **kw2)
            rc = [lib.nstl_attn_fwd(ctypes.byref(a), None), lib.nstl_last_error_string().decode(),
                  lib.nstl_attn_bwd(ctypes.byref(a), None), lib.nstl_last_error_string().decode()]
            got.append(answers(kw, {}, p, m) + rc)
    assert not any(_hip.kernel_counts().values()), "a rejected call launched"
    buf = ctypes.create_string_buffer(64)
    n = lib.nstl_attn_route_describe(None, 0, buf, 64)
    assert (n, buf.value) == (30, b"rejected: nstl_attn: null args"), (n, buf.value)
    assert lib.nstl_attn_mask_words(None) == 0 and lib.nstl_attn_bias_rows(None) == 0
    assert lib.nstl_attn_fwd(None, None) != 0 and b"null args" in lib.nstl_last_error_string()
    print(json.dumps(got))
    """, json.dumps([kw for _, kw, _ in REJECTED]), json.dumps([(p, m) for _, p, m, _ in MODES]))
    got = json.loads(out.strip().splitlines()[-1])
    assert len(got) == len(REJECTED) * len(MODES)
    bad = []
    for i, (name, _, text) in enumerate(REJECTED):
        for g in got[i * len(MODES):(i + 1) * len(MODES)]:
            fwd, bwd, words, rows, rc_f, msg_f, rc_b, msg_b = g
            if not (fwd == bwd == text and text.startswith("rejected") and words == 0 and rows == 0
                    and rc_f != 0 and rc_b != 0 and msg_f == msg_b == text[len("rejected: "):]):
                bad.append("%s: %s" % (name, g))
    assert not bad, "\n".join(bad)


def test_describe_follows_the_snprintf_convention_and_the_version():
    run_child(CHILD + """
    assert lib.nstl_version() >= 5
    a = mk(T=300, dh=120, p_drop=0.3, mask=True)
    text = b"streaming bwd DHT=128 any hi rag dm=1 rope_fast=1"
    buf = ctypes.create_string_buffer(b"#" * 63, 64)
    assert lib.nstl_attn_route_describe(ctypes.byref(a), 1, buf, 64) == len(text) and buf.value == text
    buf = ctypes.create_string_buffer(b"#" * 63, 64)
    assert lib.nstl_attn_route_describe(ctypes.byref(a), 1, buf, 10) == len(text)     # the full length
    assert buf.raw[:10] == text[:9] + b"\\0" and buf.raw[10:12] == b"##"              # 10 bytes, terminated
    assert lib.nstl_attn_route_describe(ctypes.byref(a), 1, None, 0) == len(text)     # length only
    """)

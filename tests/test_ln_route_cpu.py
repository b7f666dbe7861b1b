"""The LayerNorm routing as the host sees it, without a GPU: what nstl_ln_route_describe
answers over a literal table of argument sets.  The expected texts are written from the
rule in include/nstl.h (the table above nstl_ln_args) and the wording documented next to
nstl_ln_route_describe, not from the library's output.  All of it is host arithmetic, so
the pointers are fake (aligned integers) and nothing is launched: the entry points are
called only for arguments the table says they refuse.

Like tests/test_abi.py, every check runs in a child process: the library is never loaded
into the pytest process.

What only this table sees: a width routed to another kernel family computes the right
numbers, only slower, and engine.FP8_WIDTHS drifting from what the library accepts shows
as a late library error instead of the early ValueError."""
import json

from neurosync_trainer_lite_amd.engine import FP8_WIDTHS
from tests.test_abi import run_child

F32, BF16 = 0, 1

# D: (forward, backward) with {d} = fwd | bwd and {t} = bf16 | f32
IL = "wave-il {d} {t} V=%d G=%d"
ROUTES = {
    128: ("wave {d} {t} V=2", "wave {d} {t} V=2"),
    256: (IL % (4, 4), IL % (4, 4)),
    384: ("rowcoop fwd {t} waves=2", "rowcoop bwd {t} waves=1 groups=8"),
    512: (IL % (8, 8), IL % (8, 8)),
    768: (IL % (12, 4), IL % (12, 4)),
    896: ("rowcoop fwd {t} waves=4", "rowcoop bwd {t} waves=2 groups=4"),
    1024: (IL % (16, 8), IL % (16, 8)),
    1152: ("rowcoop fwd {t} waves=5", "rowcoop bwd {t} waves=3 groups=2"),
    1280: (IL % (20, 4), "rowcoop bwd {t} waves=3 groups=2"),
    1536: (IL % (24, 8), "rowcoop bwd {t} waves=3 groups=2"),
    1792: (IL % (28, 4), "rowcoop bwd {t} waves=4 groups=2"),
    2048: (IL % (32, 8), "rowcoop bwd {t} waves=4 groups=2"),
}

BAD_D = "rejected: nstl_ln: D=%d unsupported (a multiple of 128, 128 <= D <= 2048)"
BAD_Q8_D = "rejected: nstl_ln: the q8 / q8_scale copy (fp8) needs D in 256/512/1024 (got %d)"
BAD_Q8_F = "rejected: nstl_ln_fwd: q8 needs bf16, q8_scale and a 16-byte aligned ldq8 >= D"
BAD_Q8_B = "rejected: nstl_ln_bwd: q8 needs dbranch, bf16, q8_scale and a 16-byte aligned ldq8 >= D"
BAD_ALIGN = "rejected: nstl_ln: D=%d needs 16-byte aligned gamma/beta and 8-byte aligned rope tables"
BAD_PAIR = "rejected: nstl_ln: rows*D past 2^33 dropout elements (32-bit pair index)"
BAD_NPART = "rejected: nstl_ln_bwd: n_part (%d) must be <= rows/%d"
Q8_1024 = "wave-il {d} bf16 V=16 G=8 q8"

# (name, arguments over mk()'s defaults: bf16, 13 rows, D 1024, two masks at p 0.3, n_part 1), forward text, backward text
TABLE = [
    ("%s D %d" % (t, D), dict(dtype=dt, D=D), fwd, bwd) for D, (fwd, bwd) in ROUTES.items() for dt, t in ((BF16, "bf16"), (F32, "f32"))
] + [
    # --- the e4m3 side copy
    ("q8 D 256", dict(D=256, q8=True), IL % (4, 4) + " q8", IL % (4, 4) + " q8"),
    ("q8 D 512", dict(D=512, q8=True), IL % (8, 8) + " q8", IL % (8, 8) + " q8"),
    ("q8 D 1024", dict(q8=True), Q8_1024, Q8_1024),
    ("q8 D 1024, ldq8 1040", dict(q8=True, ldq8=1040), Q8_1024, Q8_1024),
    ("q8 D 1024, p 0", dict(q8=True, p_drop=0.0, n_masks=0), Q8_1024, Q8_1024),
    ("q8 f32", dict(dtype=F32, D=256, q8=True), BAD_Q8_F, BAD_Q8_B),
    ("q8 D 128", dict(D=128, q8=True), BAD_Q8_D % 128, BAD_Q8_D % 128),
    ("q8 D 768", dict(D=768, q8=True), BAD_Q8_D % 768, BAD_Q8_D % 768),
    ("q8 D 1536", dict(D=1536, q8=True), BAD_Q8_D % 1536, BAD_Q8_D % 1536),
    ("q8 ldq8 < D", dict(q8=True, ldq8=1008), BAD_Q8_F, BAD_Q8_B),
    ("q8 ldq8 % 16", dict(q8=True, ldq8=1032), BAD_Q8_F, BAD_Q8_B),
    ("q8 misaligned", dict(q8=True, q8_ptr=0xd008), BAD_Q8_F, BAD_Q8_B),
    ("q8 without q8_scale", dict(q8=True, q8_scale=False), BAD_Q8_F, BAD_Q8_B),
    ("q8 without dbranch", dict(q8=True, dbranch=False), Q8_1024, BAD_Q8_B),
    # --- shapes both entry points refuse
    ("D 64", dict(D=64), BAD_D % 64, BAD_D % 64),
    ("D 192", dict(D=192), BAD_D % 192, BAD_D % 192),
    ("D 2176", dict(D=2176), BAD_D % 2176, BAD_D % 2176),
    ("D 0", dict(D=0), BAD_D % 0, BAD_D % 0),
    ("rows 0", dict(rows=0), "rejected: nstl_ln: bad shape (rows=0)", "rejected: nstl_ln: bad shape (rows=0)"),
    ("dtype 7", dict(dtype=7), "rejected: nstl_ln: bad dtype", "rejected: nstl_ln: bad dtype"),
    ("p_drop 1", dict(p_drop=1.0), "rejected: nstl_ln: dropout", "rejected: nstl_ln: dropout"),
    ("p_drop -0.1", dict(p_drop=-0.1), "rejected: nstl_ln: dropout", "rejected: nstl_ln: dropout"),
    ("three masks", dict(n_masks=3), "rejected: nstl_ln: dropout", "rejected: nstl_ln: dropout"),
    # --- the 32-bit pair index: 2^33 elements are the last it reaches
    ("rows * D = 2^33, p 0.3", dict(rows=1 << 22, D=2048), IL % (32, 8), "rowcoop bwd {t} waves=4 groups=2"),
    ("rows * D past 2^33, p 0.3", dict(rows=(1 << 22) + 1, D=2048), BAD_PAIR, BAD_PAIR),
    ("rows * D past 2^33, p 0", dict(rows=(1 << 22) + 1, D=2048, p_drop=0.0), IL % (32, 8), "rowcoop bwd {t} waves=4 groups=2"),
    # --- the table alignment, at every width with a row-cooperative direction
    ("D 384, gamma at 8 bytes", dict(D=384, gamma=0x1008), BAD_ALIGN % 384, BAD_ALIGN % 384),
    ("D 384, beta at 4 bytes", dict(D=384, beta=0x1104), BAD_ALIGN % 384, BAD_ALIGN % 384),
    ("D 384, rope at 4 bytes", dict(D=384, rope=0xe004), BAD_ALIGN % 384, BAD_ALIGN % 384),
    ("D 384, rope at 8 bytes", dict(D=384, rope=0xe008), ROUTES[384][0], ROUTES[384][1]),
    ("D 1536, gamma at 8 bytes", dict(D=1536, gamma=0x1008), BAD_ALIGN % 1536, BAD_ALIGN % 1536),
    ("D 768, gamma at 4 bytes", dict(D=768, gamma=0x1004), IL % (12, 4), IL % (12, 4)),
    ("D 128, gamma and rope at 4 bytes", dict(D=128, gamma=0x1004, rope=0xe004), ROUTES[128][0], ROUTES[128][1]),
] + [
    # --- n_part <= ceil(rows / h), h = 4 at D % 256 != 0, else 8; the forward does not read n_part
    row for D, h in ((128, 4), (256, 8), (384, 4)) for rows in (3 * h, 3 * h + 1) for row in (
        ("D %d rows %d, n_part at the bound" % (D, rows), dict(D=D, rows=rows, n_part=-(-rows // h)), ROUTES[D][0], ROUTES[D][1]),
        ("D %d rows %d, n_part past the bound" % (D, rows), dict(D=D, rows=rows, n_part=-(-rows // h) + 1),
         ROUTES[D][0], BAD_NPART % (-(-rows // h) + 1, h)),
    )
] + [
    ("n_part 0", dict(n_part=0), IL % (16, 8), "rejected: nstl_ln_bwd: partials"),
]

CHILD = """
    import ctypes, json
    from neurosync_trainer_lite_amd import _hip
    lib = _hip.lib()

    def mk(dtype=1, rows=13, D=1024, n_masks=2, p_drop=0.3, n_part=1, q8=False, ldq8=None, q8_ptr=0xd000, q8_scale=True,
           dbranch=True, gamma=0x1000, beta=0x1100, rope=None):
        a = _hip.ln_args(dtype, rows, D, n_masks, p_drop, 11, 12, n_part=n_part)
        a.x, a.y, a.gamma, a.beta = 0x2000, 0x3000, gamma, beta
        a.s_out, a.out, a.mean, a.rstd = 0x4000, 0x5000, 0x6000, 0x7000
        a.s_in, a.dout, a.ds, a.dbranch = 0x4000, 0x8000, 0x8000, 0x9000 if dbranch else None
        a.dgamma_part, a.dbeta_part, a.dbranch_part = 0xa000, 0xb000, 0xc000
        if rope is not None:
            a.rot_out, a.rope_cos, a.rope_sin, a.rope_T = 0xf000, rope, rope + 0x800, 4
        if q8:
            a.q8, a.ldq8, a.q8_scale = q8_ptr, D if ldq8 is None else ldq8, 0xd800 if q8_scale else None
        return a

    def answers(kw):
        a = mk(**kw)
        got = [_hip.ln_route(a), _hip.ln_route(a, backward=True)]
        # what the table says is refused is refused by the entry point, in the same words
        for text, fn in zip(got, (lib.nstl_ln_fwd, lib.nstl_ln_bwd)):
            if text.startswith("rejected: "):
                rc = fn(ctypes.byref(a), None)
                got.append([rc != 0, lib.nstl_last_error_string().decode()])
            else:
                got.append(None)
        return got
"""


def fmt(text, d, kw):
    return text.format(d=d, t="f32" if kw.get("dtype", BF16) == F32 else "bf16")


def test_route_over_the_table():
    out = run_child(CHILD + """
    print(json.dumps([answers(kw) for kw in json.loads(sys.argv[1])]))
    """, json.dumps([kw for _, kw, _, _ in TABLE]))
    got = json.loads(out.strip().splitlines()[-1])
    assert len(got) == len(TABLE)
    bad = []
    for (name, kw, fwd, bwd), (g_fwd, g_bwd, e_fwd, e_bwd) in zip(TABLE, got):
        for want, g, e in ((fmt(fwd, "fwd", kw), g_fwd, e_fwd), (fmt(bwd, "bwd", kw), g_bwd, e_bwd)):
            entry = [True, want[len("rejected: "):]] if want.startswith("rejected: ") else None
            if g != want or e != entry:
                bad.append("%s: %r %r, expected %r %r" % (name, g, e, want, entry))
    assert not bad, "\n".join(bad)


def test_fp8_widths_are_the_widths_that_take_q8():
    widths = list(range(128, 2049, 128))
    out = run_child(CHILD + """
    print(json.dumps([[D, _hip.ln_route(mk(D=D, q8=True)), _hip.ln_route(mk(D=D, q8=True), backward=True)]
                      for D in json.loads(sys.argv[1])]))
    """, json.dumps(widths))
    got = json.loads(out.strip().splitlines()[-1])
    assert [D for D, _, _ in got] == widths
    for backward in (0, 1):
        ok = [D for D, *texts in got if not texts[backward].startswith("rejected")]
        assert tuple(ok) == tuple(FP8_WIDTHS), (backward, got)
    assert all(texts[0].endswith(" q8") and texts[1].endswith(" q8") for D, *texts in got if D in FP8_WIDTHS), got


def test_describe_follows_the_snprintf_convention_and_the_version():
    run_child(CHILD + """
    assert lib.nstl_version() >= 8
    a = mk(D=1152)
    text = b"rowcoop bwd bf16 waves=3 groups=2"
    buf = ctypes.create_string_buffer(b"#" * 63, 64)
    assert lib.nstl_ln_route_describe(ctypes.byref(a), 1, buf, 64) == len(text) and buf.value == text
    buf = ctypes.create_string_buffer(b"#" * 63, 64)
    assert lib.nstl_ln_route_describe(ctypes.byref(a), 1, buf, 10) == len(text)     # the full length
    assert buf.raw[:10] == text[:9] + b"\\0" and buf.raw[10:12] == b"##"            # 10 bytes, terminated
    assert lib.nstl_ln_route_describe(ctypes.byref(a), 1, None, 0) == len(text)     # length only
    buf = ctypes.create_string_buffer(64)
    n = lib.nstl_ln_route_describe(None, 0, buf, 64)
    assert (n, buf.value) == (28, b"rejected: nstl_ln: null args"), (n, buf.value)
    assert lib.nstl_ln_fwd(None, None) != 0 and b"null args" in lib.nstl_last_error_string()
    assert lib.nstl_ln_bwd(None, None) != 0 and b"null args" in lib.nstl_last_error_string()
    """)

"""The GEMM routing as the host sees it, without a GPU: what the two size queries
(nstl_gemm_colsum_rows, nstl_gemm_relu_mask_words) answer over a literal table of
argument sets, and the calls nstl_gemm / nstl_gemm_grouped reject before they
route anything.  The queries are pure host code, so the pointers are fake
(16-byte aligned integers) and no row reaches a launch.

Like tests/test_abi.py, every check runs in a child process: the library is never
loaded into the pytest process.

The queries answer for the ring kernels (csrc/gemm.hip route()): bf16 needs 32
tiles of 256 x 256 and K % 64 == 0, fp8 any shape with K % 64 == 0; a call
nstl_gemm itself rejects answers 0 (rows marked REJECTED: a build before the
one-route refactor answered those from the shape alone)."""
import json

from tests.test_abi import run_child

F32, BF16, FP8 = 0, 1, 2
NONE, BIAS, RELU_DROP, ROPE, DRELU = 0, 1, 2, 3, 4
REJECTED = "rejected"

# (name, arguments over the defaults of CHILD's mk(): bf16 TT 2048 x 1024 x 1024, bf16 C, beta 0), rows, words)
TABLE = [
    # --- bf16: the ring kernel's 32-tile rule
    ("32 tiles relu_drop", dict(epilogue=RELU_DROP), 0, 32768),
    ("32 tiles drelu", dict(epilogue=DRELU), 16, 32768),
    ("32 tiles 8192x256 drelu", dict(M=8192, N=256, epilogue=DRELU), 64, 32768),
    ("31 tiles relu_drop", dict(M=7936, N=256, epilogue=RELU_DROP), 0, 0),
    ("31 tiles drelu", dict(M=7936, N=256, epilogue=DRELU), 0, 0),
    # 28 whole tiles run on the 4-wave kernel, which would honour a mask: the queries still answer 0
    ("28 whole tiles relu_drop", dict(M=1792, epilogue=RELU_DROP), 0, 0),
    ("28 whole tiles drelu", dict(M=1792, epilogue=DRELU), 0, 0),
    ("M = 2100 relu_drop", dict(M=2100, epilogue=RELU_DROP), 0, 33792),
    ("M = 2100 drelu", dict(M=2100, epilogue=DRELU), 17, 33792),
    ("N = 1000 relu_drop", dict(N=1000, epilogue=RELU_DROP), 0, 32000),
    ("N = 1000 drelu", dict(N=1000, epilogue=DRELU), 16, 32000),
    ("odd N relu_drop", dict(N=1001, epilogue=RELU_DROP), 0, 0),
    ("odd N drelu", dict(N=1001, epilogue=DRELU), 16, 32256),
    ("K = 1000 drelu", dict(K=1000, epilogue=DRELU), 0, 0),
    ("M = 255 drelu", dict(M=255, N=16384, epilogue=DRELU), 0, 0),
    # --- beta, output type, split-K
    ("beta 1 relu_drop", dict(beta=1.0, epilogue=RELU_DROP), 0, 0),
    ("beta 1 drelu", dict(beta=1.0, epilogue=DRELU), 0, 0),
    ("f32 C relu_drop", dict(c_dtype=F32, epilogue=RELU_DROP), 0, 0),
    ("f32 C drelu", dict(c_dtype=F32, epilogue=DRELU), 0, 0),
    ("split_k 2 relu_drop", dict(split_k=2, epilogue=RELU_DROP), 0, 0),
    ("split_k 2 drelu", dict(split_k=2, epilogue=DRELU), 0, 0),
    ("split_k 2 none", dict(split_k=2, workspace=True), 0, 0),
    # --- the other epilogues and layouts
    ("none", dict(), 0, 0),
    ("bias", dict(epilogue=BIAS), 0, 0),
    ("rope", dict(epilogue=ROPE), 0, 0),
    ("TN drelu (dX)", dict(b_kmajor=0, epilogue=DRELU), 16, 32768),
    ("NN drelu", dict(a_kmajor=0, b_kmajor=0, epilogue=DRELU), 16, 32768),
    ("drelu with keep bits", dict(epilogue=DRELU, relu_mask=True), 16, 32768),
    ("relu_drop with keep bits", dict(epilogue=RELU_DROP, relu_mask=True), 0, 32768),
    ("drelu with colsum_part", dict(epilogue=DRELU, colsum_part=True), 16, 32768),
    # --- f32 operands: the 128 kernel, no side outputs
    ("f32 relu_drop", dict(dtype=F32, c_dtype=F32, epilogue=RELU_DROP), 0, 0),
    ("f32 drelu", dict(dtype=F32, c_dtype=F32, epilogue=DRELU), 0, 0),
    # --- fp8: the fp8 ring kernel at any tile count
    ("fp8 256^3 relu_drop", dict(dtype=FP8, M=256, N=256, K=256, epilogue=RELU_DROP), 0, 1024),
    ("fp8 256^3 drelu", dict(dtype=FP8, M=256, N=256, K=256, epilogue=DRELU), 2, 1024),
    ("fp8 2048x1024x1024 drelu", dict(dtype=FP8, epilogue=DRELU), 16, 32768),
    ("fp8 M = 100 drelu", dict(dtype=FP8, M=100, epilogue=DRELU), 1, 2048),
    ("fp8 odd N relu_drop", dict(dtype=FP8, N=1001, epilogue=RELU_DROP), 0, 0),
    ("fp8 f32 C none", dict(dtype=FP8, c_dtype=F32), 0, 0),
    ("fp8 f32 C drelu", dict(dtype=FP8, c_dtype=F32, epilogue=DRELU), 0, 0),
    ("fp8 beta 1 drelu", dict(dtype=FP8, beta=1.0, epilogue=DRELU), 0, 0),
    ("fp8 bias", dict(dtype=FP8, epilogue=BIAS), 0, 0),
    ("fp8 split_k 2 drelu", dict(dtype=FP8, split_k=2, epilogue=DRELU), 0, 0),
    # --- calls nstl_gemm rejects: 0
    ("null args", None, 0, 0),
    ("bad dtype", dict(dtype=7, epilogue=DRELU), 0, 0),
    ("lda < K", dict(lda=512, epilogue=DRELU), 0, 0),
    ("misaligned A", dict(A=0x1008, epilogue=DRELU), 0, 0),
    ("drelu without aux", dict(epilogue=DRELU, aux=False), 0, 0),
    (REJECTED + ": fp8 K % 64 != 0 relu_drop", dict(dtype=FP8, K=1000, lda=1008, ldb=1008, epilogue=RELU_DROP), 0, 0),
    (REJECTED + ": fp8 K % 64 != 0 drelu", dict(dtype=FP8, K=1000, lda=1008, ldb=1008, epilogue=DRELU), 0, 0),
    (REJECTED + ": fp8 without row scales", dict(dtype=FP8, scales=False, epilogue=DRELU), 0, 0),
    (REJECTED + ": fp8 with an MN-major B", dict(dtype=FP8, b_kmajor=0, epilogue=DRELU), 0, 0),
    (REJECTED + ": fp8 sq_part", dict(dtype=FP8, sq_part=True, epilogue=DRELU), 0, 0),
    (REJECTED + ": fp8 relu_drop with colsum_part", dict(dtype=FP8, colsum_part=True, epilogue=RELU_DROP), 0, 0),
    (REJECTED + ": bf16 sq_part", dict(sq_part=True, epilogue=DRELU), 0, 0),
    (REJECTED + ": bf16 relu_drop with colsum_part", dict(colsum_part=True, epilogue=RELU_DROP), 0, 0),
]

# nstl_gemm / nstl_gemm_grouped calls that fail in validation: (name, [problems], grouped, fragment of the error)
FAILS = [
    ("bad dtype", [dict(dtype=7)], False, "dtype"),
    ("lda < K", [dict(lda=512)], False, "lda"),
    ("empty problem", [dict(M=0)], False, "empty problem"),
    ("sq_part outside a group", [dict(sq_part=True)], False, "nstl_gemm_grouped only"),
    ("colsum_part without dReLU", [dict(colsum_part=True)], False, "colsum_part"),
    ("keep bits under 32 tiles, odd K", [dict(M=1792, K=1000, epilogue=RELU_DROP, relu_mask=True)], False, "256 kernel"),
    ("fp8 K % 64", [dict(dtype=FP8, K=1000, lda=1008, ldb=1008)], False, "K % 64"),
    ("fp8 layout", [dict(dtype=FP8, b_kmajor=0)], False, "K-major"),
    ("fp8 scales", [dict(dtype=FP8, scales=False)], False, "row scales"),
    ("fp8 split-K", [dict(dtype=FP8, split_k=2)], False, "no split-K"),
    ("fp8 beta", [dict(dtype=FP8, beta=1.0, epilogue=BIAS)], False, "FP8 supports"),
    ("group of 17", [dict(a_kmajor=0, b_kmajor=0, c_dtype=F32)] * 17, True, "1..16 problems"),
    ("group of 0", [], True, "1..16 problems"),
    ("group with an empty problem", [dict(), dict(N=0)], True, "empty problem"),
    ("group with a small problem", [dict(), dict(M=128)], True, "256-kernel"),
    ("group with mixed layouts", [dict(), dict(b_kmajor=0)], True, "differs"),
    ("group with two RoPE tables", [dict(epilogue=ROPE), dict(epilogue=ROPE, rope_T=64)], True, "share one table"),
    ("group with split-K", [dict(), dict(split_k=2, workspace=True)], True, "no split-K"),
]

CHILD = """
    import ctypes, json
    from neurosync_trainer_lite_amd import _hip
    lib = _hip.lib()

    def mk(dtype=1, c_dtype=1, M=2048, N=1024, K=1024, a_kmajor=1, b_kmajor=1, lda=None, ldb=None, A=0x1000,
           beta=0.0, epilogue=0, aux=True, split_k=1, workspace=False, colsum_part=False, relu_mask=False,
           scales=True, sq_part=False, rope_T=128):
        a = _hip.GemmArgs()
        a.dtype, a.c_dtype, a.a_kmajor, a.b_kmajor = dtype, c_dtype, a_kmajor, b_kmajor
        a.A, a.B, a.C = A, 0x2000, 0x3000
        a.lda = lda if lda is not None else (K if a_kmajor else M)
        a.ldb = ldb if ldb is not None else (K if b_kmajor else N)
        a.ldc = N
        a.M, a.N, a.K = M, N, K
        a.alpha, a.beta, a.epilogue = 1.0, beta, epilogue
        a.bias = 0x4000
        if epilogue == 4 and aux:
            a.aux, a.ld_aux = 0x5000, N
        a.p_drop, a.seed = 0.1, 7
        if epilogue == 3:
            a.rope_cos, a.rope_sin, a.rope_T, a.rope_dim, a.rope_cols = 0x6000, 0x7000, rope_T, 64, 1024
        a.split_k = split_k
        if workspace:
            a.workspace, a.workspace_bytes = 0x8000, split_k * M * N * 4
        a.colsum_part = 0x9000 if colsum_part else None
        a.relu_mask = 0xa000 if relu_mask else None
        if dtype == 2 and scales:
            a.a_scale, a.b_scale = 0xb000, 0xc000
        a.sq_part = 0xd000 if sq_part else None
        return a
"""


def test_size_queries_over_the_routing_table():
    out = run_child(CHILD + """
    got = []
    for kw in json.loads(sys.argv[1]):
        ref = ctypes.byref(mk(**kw)) if kw is not None else None
        got.append([lib.nstl_gemm_colsum_rows(ref), lib.nstl_gemm_relu_mask_words(ref)])
    print(json.dumps(got))
    """, json.dumps([kw for _, kw, _, _ in TABLE]))
    got = json.loads(out.strip().splitlines()[-1])
    bad = ["%s: (rows, words) = %s, expected %s" % (name, tuple(g), (rows, words))
           for (name, _, rows, words), g in zip(TABLE, got) if tuple(g) != (rows, words)]
    assert len(got) == len(TABLE) and not bad, "\n".join(bad)


def test_calls_rejected_before_routing():
    out = run_child(CHILD + """
    _hip.kernel_counts_reset()
    got = []
    for probs, grouped in json.loads(sys.argv[1]):
        arr = (_hip.GemmArgs * max(len(probs), 1))(*[mk(**kw) for kw in probs])
        rc = lib.nstl_gemm_grouped(arr, len(probs), None) if grouped else lib.nstl_gemm(arr, None)
        got.append([rc, lib.nstl_last_error_string().decode()])
    assert not any(_hip.kernel_counts().values()), "a rejected call launched"
    print(json.dumps(got))
    """, json.dumps([(probs, grouped) for _, probs, grouped, _ in FAILS]))
    got = json.loads(out.strip().splitlines()[-1])
    bad = ["%s: rc %d, %r (expected an error with %r)" % (name, rc, msg, frag)
           for (name, _, _, frag), (rc, msg) in zip(FAILS, got) if rc == 0 or frag not in msg]
    assert len(got) == len(FAILS) and not bad, "\n".join(bad)

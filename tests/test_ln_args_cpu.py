"""_hip.ln_args / ln_set on CPU tensors: every operand is checked against the extent the
call addresses and the element type it is read as before anything could be launched, and
the struct keeps its tensors alive.  No library call: ln_set is Python arithmetic on the
tensors' storages."""
import gc
import weakref

import pytest
import torch

from neurosync_trainer_lite_amd import _hip as K

ROWS, D, N_PART, ROPE_T, LDQ8 = 5, 256, 3, 4, 272
BF, F32, E4 = torch.bfloat16, torch.float32, torch.float8_e4m3fn

# operand: (elements the call addresses, element type in a bf16 call)
OPERANDS = dict(
    [(n, (ROWS * D, BF)) for n in ("x", "y", "s_out", "out", "rot_out", "s_in", "dbranch", "dout2")]
    + [(n, (ROWS * D, F32)) for n in ("dout", "ds")]
    + [(n, (ROWS, F32)) for n in ("mean", "rstd", "q8_scale")]
    + [(n, (D, F32)) for n in ("gamma", "beta")]
    + [(n, (ROPE_T * (D // 2), F32)) for n in ("rope_cos", "rope_sin")]
    + [(n, (N_PART * D, F32)) for n in ("dgamma_part", "dbeta_part", "dbranch_part")])


def args(dtype=K.BF16):
    return K.ln_args(dtype, ROWS, D, 2, 0.3, 11, 12, n_part=N_PART)


def test_the_table_names_every_pointer_of_the_struct():
    scalars = {"dtype", "rows", "D", "n_masks", "p_drop", "seed1", "seed2", "eps", "rope_T", "n_part", "ldq8"}
    assert set(OPERANDS) | {"q8"} == {f[0] for f in K.LnArgs._fields_} - scalars


@pytest.mark.parametrize("name", sorted(OPERANDS))
def test_operand_extent_and_dtype(name):
    n, dt = OPERANDS[name]
    a = args()
    t = torch.zeros(n, dtype=dt)
    assert K.ln_set(a, rope_T=ROPE_T, **{name: t}) is a
    assert getattr(a, name) == t.data_ptr()
    # the same storage seen from one element in, and a tensor one element short
    for short in (torch.zeros(n + 1, dtype=dt)[2:], torch.zeros(n - 1, dtype=dt)):
        b = args()
        with pytest.raises(ValueError, match=r"nstl_ln %s \[" % name):
            K.ln_set(b, rope_T=ROPE_T, **{name: short})
        assert getattr(b, name) is None and name not in b.tensors
    other = F32 if dt == BF else BF
    with pytest.raises(TypeError, match="nstl_ln %s " % name):
        K.ln_set(args(), rope_T=ROPE_T, **{name: torch.zeros(n, dtype=other)})
    # an f32 call reads the dtype operands as f32
    if dt == BF:
        K.ln_set(args(K.F32), **{name: torch.zeros(n, dtype=F32)})
        with pytest.raises(TypeError, match="nstl_ln %s " % name):
            K.ln_set(args(K.F32), **{name: t})
    K.ln_set(a, **{name: None})
    assert getattr(a, name) is None and name not in a.tensors


def test_q8_takes_its_stride_from_the_tensor():
    a = args()
    q = torch.zeros(ROWS, LDQ8, dtype=E4)
    K.ln_set(a, q8=q[:, :D])
    assert (a.q8, a.ldq8) == (q.data_ptr(), LDQ8)
    K.ln_set(a, q8=torch.zeros((ROWS - 1) * LDQ8 + D, dtype=E4).as_strided((ROWS, D), (LDQ8, 1)))   # the last row ends the storage
    # one element short of the call's last row (torch lets a view name only the rows the storage holds)
    with pytest.raises(ValueError, match=r"nstl_ln q8 \[rows\]\[ldq8\]"):
        K.ln_set(args(), q8=torch.zeros((ROWS - 1) * LDQ8 + D - 1, dtype=E4).as_strided((ROWS - 1, D), (LDQ8, 1)))
    with pytest.raises(TypeError, match="nstl_ln q8 "):
        K.ln_set(args(), q8=torch.zeros(ROWS, LDQ8, dtype=torch.uint8))


def test_unknown_operand_is_a_type_error():
    with pytest.raises(TypeError, match="unknown operand 'gama'"):
        K.ln_set(args(), gama=torch.zeros(D))


def test_the_struct_keeps_its_tensors_alive():
    a = args()
    t = torch.zeros(D)
    ref, ptr = weakref.ref(t), t.data_ptr()
    K.ln_set(a, gamma=t.detach().float().contiguous())   # f32 already: the same tensor object or a view of it
    K.ln_set(a, beta=t)
    del t
    gc.collect()
    assert ref() is not None and a.beta == ptr
    # a temporary nothing else refers to
    K.ln_set(a, mean=torch.zeros(ROWS))
    tmp = weakref.ref(a.tensors["mean"])
    gc.collect()
    assert tmp() is not None and tmp().data_ptr() == a.mean
    del a
    gc.collect()
    assert ref() is None and tmp() is None

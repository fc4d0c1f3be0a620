"""CPU: the Python binding's signature tables against the two C headers, and load() binding every table on every library object
it opens.  The header parser is the Rust binding's (tests/test_rust_shims.py)."""
import ctypes
import importlib.util
import os
import re

import pytest

from test_rust_shims import _c_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POINTER, I32, U32, I64, U64 = "pointer", "int32", "uint32", "int64", "uint64"
C_INTEGERS = {"int": I32, "uint32_t": U32, "int64_t": I64, "uint64_t": U64}
PY_INTEGERS = {ctypes.c_int: I32, ctypes.c_uint32: U32, ctypes.c_int64: I64, ctypes.c_uint64: U64}


def c_class(ctype):
    if "*" in ctype:
        return POINTER
    if re.fullmatch(r"zk_[a-z0-9_]+_t", ctype):         # the enums
        return I32
    return C_INTEGERS[ctype]


def py_class(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return POINTER
    return PY_INTEGERS[t]


def tables(zk):
    return [zk.SIGNATURES, zk.PROVER_SIGNATURES, zk.ark_serialize.SIGNATURES, zk.groth16.SIGNATURES, zk.halo2.SIGNATURES,
            zk.poseidon.SIGNATURES, zk.encryption.SIGNATURES]


def accessors(zk):
    """the legacy accessors, each with one entry point of its module and arguments that name no memory"""
    return [(zk.load, "zk_field_inverse", (0, None, None)),
            (zk.halo2._plib, "zk_batch_invert_device", (0, None, 1, None)),
            (zk.poseidon._plib, "zk_vec_add_scalar_device", (0, None, None, 1, None, None)),
            (lambda: zk.poseidon._bind(zk.load()), "zk_vec_add_scalar_device", (0, None, None, 1, None, None)),
            (zk.groth16._lib, "zk_r1cs_matvec_device", (0, None, None, 1, None)),
            (zk.ark_serialize._lib, "zk_ark_scalars_encode", (0, None, 1, None)),
            (zk.encryption._elib, "zk_encrypt_witness_device", (zk.FR_BLS12_381, None, 1, 1, None, None, None, None, None, None))]


def test_tables_match_headers():
    import contangle_zkcp_amd as zk
    c = _c_params()
    names = [n for t in tables(zk) for n in t]
    assert len(names) == len(set(names)), "an entry point sits in two tables"
    assert sorted(names) == sorted(c), (sorted(set(c) - set(names)), sorted(set(names) - set(c)))
    checked = 0
    for table in tables(zk):
        for name, argtypes in table.items():
            assert len(argtypes) == len(c[name]), (name, c[name], argtypes)
            for i, (ct, pt) in enumerate(zip(c[name], argtypes)):
                assert c_class(ct) == py_class(pt), (name, i, ct, pt)
                checked += 1
    assert checked > 400
    # the one function that does not return a status, and nothing else
    assert zk.RETURNS == {"zk_strerror": ctypes.c_char_p}
    assert zk.EXPORTS == list(zk.SIGNATURES)


def fully_bound(zk, lib):
    for table in tables(zk):
        for name, argtypes in table.items():
            fn = getattr(lib, name)
            assert list(fn.argtypes) == list(argtypes), name
            assert fn.restype is (ctypes.c_char_p if name == "zk_strerror" else ctypes.c_int), name
    return True


@pytest.fixture(scope="module")
def emu():
    spec = importlib.util.spec_from_file_location("zk_build", os.path.join(ROOT, "contangle-zkcp_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    import contangle_zkcp_amd as zk
    saved = zk._lib
    yield b.build_emu()
    zk._lib = saved


def test_every_library_object_is_bound(emu):
    import contangle_zkcp_amd as zk
    first = zk.load(path=emu)
    assert fully_bound(zk, first) and zk.load() is first
    zk._lib = None
    second = zk.load(path=emu)
    assert second is not first and fully_bound(zk, second)
    for accessor, _, _ in accessors(zk):
        zk._lib = None
        saved, zk.LIB_PATH = zk.LIB_PATH, emu             # the accessors take no path: they open LIB_PATH
        try:
            lib = accessor()
        finally:
            zk.LIB_PATH = saved
        assert lib is zk._lib and lib is not second and fully_bound(zk, lib)


def test_raw_calls_return_the_status_and_call_raises(emu):
    import contangle_zkcp_amd as zk
    zk._lib = None
    zk.load(path=emu)
    for accessor, name, args in accessors(zk):
        st = getattr(accessor(), name)(*args)
        assert isinstance(st, int) and st < 0, (name, st)
        with pytest.raises(zk.ZkError) as e:
            zk._call(name, *args)
        assert e.value.status == st and str(e.value).startswith(name + " failed: ") and str(e.value).endswith("(%d)" % st)

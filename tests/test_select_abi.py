"""CPU checks of the selective unpack's boundary (no GPU): the header
declares capnp_gpu_unpack_batch_select, the library exports it, the binding
lists it, and a call without a context is refused."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "capnp_gpu_unpack_batch_select"


def test_header_declares_select():
    src = open(os.path.join(ROOT, "include", "capnp_packed.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"capnp_status\s+" + NAME + r"\s*\(([^;]*)\)\s*;", src)
    assert m, "not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 14
    # the offsets of the output are written by the call; the ids and the index are inputs
    assert any(a.startswith("const uint64_t*") and a.endswith("d_ids") for a in args)
    assert any(a.startswith("const uint32_t*") and a.endswith("d_sync") for a in args)
    assert any(a.startswith("uint64_t*") and a.endswith("d_out_word_off") for a in args)


def test_library_exports_select():
    from capnp_amd import _lib
    assert NAME in _lib.EXPORTS
    assert hasattr(_lib.lib(), NAME)
    assert NAME in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 6 and _lib.lib().capnp_abi_version() == 6  # additions only


def test_select_refuses_a_null_context():
    from capnp_amd import _lib
    L = _lib.lib()
    st = L.capnp_gpu_unpack_batch_select(None, None, None, None, 0, None, 0, None, None, 0, None,
                                         None, None, None)
    assert st == 64


def test_python_mirror_has_select():
    from capnp_amd import Context
    assert callable(Context.unpack_select_into) and callable(Context.unpack_select)

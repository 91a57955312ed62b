"""CPU: the observables interface (include/nls.h "Observables") is declared, exported and
bound consistently, inside ABI 6, and the new kernels keep everything in registers and LDS
(code-object metadata only)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nls.h")
FUNCS = ("nls_observe", "nls_monitor", "nls_observe_async", "nls_monitor_read")
FIELDS = ("step", "mass", "kinetic", "p4", "p6", "vel2", "potential", "energy", "max_abs2", "nonfinite")

import nls_amd  # the project's own binding: a failed import is an error, not a skip


def test_header_declares_the_interface():
    txt = open(HEADER).read()
    for f in FUNCS:
        assert re.search(rf"^int {f}\(nls_handle \*", txt, re.M), f
    assert re.search(r"^#define NLS_OBS_NFIELDS 10$", txt, re.M)
    m = re.search(r"typedef struct nls_observables \{(.*?)\} nls_observables;", txt, re.S)
    assert m, "struct nls_observables"
    names = re.findall(r"\b([a-z_0-9]+)\s*[,;]", m.group(1))
    assert tuple(names) == FIELDS
    assert re.search(r"^#define NLS_ABI_VERSION 6$", txt, re.M)
    # the caveats a caller must know
    assert "THIS RANK'S SLAB" in txt and "not Hamiltonian" in txt and "No conservation is claimed" in txt


def test_library_exports_the_functions_in_abi_6():
    out = subprocess.run(["nm", "-D", "--defined-only", nls_amd.lib_path()], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (nls_\w+)", out))
    assert set(FUNCS) <= exported
    assert set(FUNCS) <= set(nls_amd.EXPORTED_SYMBOLS)
    assert nls_amd.lib().nls_abi_version() == 6


def test_binding_struct_layout():
    assert nls_amd.OBS_FIELDS == FIELDS
    assert C.sizeof(nls_amd.Observables) == 80
    assert tuple(n for n, _t in nls_amd.Observables._fields_) == nls_amd.OBS_FIELDS
    assert all(t is C.c_double for _n, t in nls_amd.Observables._fields_)


def test_null_handle_rejected_without_a_device():
    L = nls_amd.lib()
    o = nls_amd.Observables()
    n = C.c_uint64(7)
    assert L.nls_observe(None, 0.0, C.byref(o)) == -1
    assert L.nls_monitor(None, 1, 4) == -1
    assert L.nls_observe_async(None, 0.0) == -1
    assert L.nls_monitor_read(None, None, 0, C.byref(n)) == -1 and n.value == 7


@pytest.mark.skipif(not codeobj.available(), reason="ROCm llvm tools missing")
def test_observe_kernels_use_no_private_segment(tmp_path):
    """k_observe (every instantiation: 2 operators x 2 dimensions x the equation classes
    the ten equations need) and k_observe_finish: private_segment_fixed_size == 0 and no
    VGPR spill in the code-object metadata."""
    seen = []
    for co in codeobj.gfx950_objects(nls_amd.lib_path(), str(tmp_path)):
        for name, meta in codeobj.metadata(co).items():
            if "k_observe" not in name:
                continue
            seen.append(name)
            assert int(meta.get("private_segment_fixed_size", "0")) == 0, name
            assert str(meta.get("vgpr_spill_count", "0")) == "0", name
    assert sum("k_observe_finish" in n for n in seen) == 1
    # complex: iso {w = 1, w = m} + ani {w = m}; real: iso {4 potentials} + ani {KG}; x {2D, 3D}
    assert sum("k_observe_finish" not in n for n in seen) == 16

"""CPU tests of the drop-in boundary: libmgicp.so loads, exports exactly the symbols its two C-ABI
headers declare (product and debug), the drop-in needs the product header alone, its ctypes mirrors match the header's structs, and nothing silently falls back to
CPU compute when no GPU is present."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mi355x_gicp.h")
DEBUG_HEADER = os.path.join(ROOT, "include", "mi355x_gicp_debug.h")


def _struct_fields(name):
    text = open(HEADER).read()
    m = re.search(r"typedef struct \{([^{}]*)\}\s*" + name + ";", text, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(n.strip(), typ) for n in names.split(",")]
    return fields


def _nm(flag, path):
    """Names `nm <flag> path` lists (last column)."""
    out = subprocess.run(["nm", *flag.split(), path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_library_exports_every_header_symbol():
    from leica_point_cloud_processing_amd import _lib

    lib = _lib.load()
    syms = _lib.header_symbols()
    assert len(syms) >= 20
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert set(syms) == set(_lib._SIGNATURES), "ctypes signature table out of sync with the header"
    # ... and nothing else (csrc/libmgicp.map): no launcher, kernel stub or template instance that another
    # library of the host process could interpose or collide with
    exported = _nm("-D --defined-only", _lib.LIB_PATH)
    assert exported == set(syms), sorted(exported ^ set(syms))


def test_headers_split_product_from_debug():
    """include/mi355x_gicp.h is the drop-in; every test / bench hook is in mi355x_gicp_debug.h."""
    from leica_point_cloud_processing_amd import _lib

    product = set(_lib.header_symbols(_lib.HEADER_PATH))
    debug = set(_lib.header_symbols(_lib.DEBUG_HEADER_PATH))
    assert not product & debug, sorted(product & debug)
    assert product | debug == set(_lib.header_symbols())
    assert product and not [s for s in product if s.startswith("mgicp_debug_")]
    assert debug == {s for s in _lib._SIGNATURES if s.startswith("mgicp_debug_")} | {"mgicp_set_profiling"}


@pytest.mark.parametrize("cname,pyname", [("mgicp_params", "MgicpParams"), ("mgicp_result", "MgicpResult")])
def test_struct_layout_matches_header(cname, pyname):
    from leica_point_cloud_processing_amd import _lib

    cls = getattr(_lib, pyname)
    hdr = _struct_fields(cname)
    py = [(n, t) for n, t in cls._fields_]
    assert [n for n, _ in hdr] == [n for n, _ in py]
    cmap = {"int": ctypes.c_int, "double": ctypes.c_double}
    for (n, ct), (_, pt) in zip(hdr, py):
        assert cmap[ct] == pt, n


def test_header_is_plain_c():
    for header in (HEADER, DEBUG_HEADER):
        text = open(header).read()
        assert 'extern "C"' in text, header
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # declarations only, not the docs
        for banned in ("torch", "hipStream_t", "Eigen", "pcl::", "std::", "#include <hip"):
            assert banned not in text, (header, banned)
        # each header on its own (the debug header includes what it needs) through a C99 compiler
        r = subprocess.run(["gcc", "-x", "c", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", header],
                           capture_output=True, text=True)
        assert r.returncode == 0, (header, r.stderr)


def test_drop_in_uses_the_product_header_only():
    """What an integrator compiles and links -- the adapter sources and the C-ABI example -- includes
    mi355x_gicp.h alone of the engine's headers, names no debug hook, and its binaries need no mgicp_* symbol
    outside that header."""
    import glob

    from leica_point_cloud_processing_amd import _lib

    product = set(_lib.header_symbols(_lib.HEADER_PATH))
    debug = set(_lib.header_symbols(_lib.DEBUG_HEADER_PATH))
    adapter = os.path.join(ROOT, "adapter")
    sources = sorted(glob.glob(os.path.join(adapter, "*.cpp")) + glob.glob(os.path.join(adapter, "*.h")))
    assert os.path.join(adapter, "cabi_example.cpp") in sources and len(sources) >= 5
    for path in sources:
        text = open(path).read()
        assert "mi355x_gicp_debug.h" not in text, path
        # of the engine's headers the product header alone; the adapter's own headers (the shared helper
        # context) are part of what the integrator compiles and pass through this same loop
        own = {os.path.basename(s) for s in sources}
        assert set(re.findall(r'#include\s*[<"]([^">]*mi355x[^">]*)[">]', text)) - own <= {"mi355x_gicp.h"}, path
        named = set(re.findall(r"\bmgicp_[a-z_0-9]+", text))
        assert not named & debug, (path, sorted(named & debug))
    subprocess.run(["make", "-s", "-C", ROOT, "adapter-example", "adapter-replay", "fod-replay"], check=True,
                   capture_output=True, text=True)
    for exe in ("cabi_example", os.path.join("build", "replay_test_gicp_alignment"),
                os.path.join("build", "replay_test_fod_detector")):
        needed = {s for s in _nm("-u", os.path.join(adapter, exe)) if s.startswith("mgicp_")}
        assert needed and needed <= product, (exe, sorted(needed - product))


def test_default_params_match_reference():
    """GICPAlignment ctor defaults (src/GICPAlignment.cpp:29-32) + PCL GICP defaults."""
    from leica_point_cloud_processing_amd import _lib

    p = _lib.default_params()
    assert (p.max_iter, p.k, p.max_inner_iter) == (100, 20, 20)
    assert (p.tf_eps, p.rot_eps, p.max_corr_dist, p.gicp_eps) == (4e-3, 2e-3, 4e-2, 1e-3)


def test_no_cpu_fallback_without_gpu():
    """On a machine without a GPU the engine refuses to run instead of computing on the CPU."""
    from leica_point_cloud_processing_amd import _lib
    from leica_point_cloud_processing_amd.engine import GICPEngine

    n = ctypes.c_int(0)
    rc = _lib.load().mgicp_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.MgicpError):
        GICPEngine()


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: no product module may reference it."""
    pkg = os.path.join(ROOT, "leica_point_cloud_processing_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'#include\s*["<][^">]*gicp_ref', text), f
                assert not re.search(r"\bref_[a-z_]+\s*\(", text), f
                assert not re.search(r"^\s*(from oracle|import oracle)", text, re.M), f
                assert "libgicp_ref" not in text, f


@pytest.mark.gpu
def test_cabi_example_plain_cpp_host():
    """adapter/cabi_example (g++, no HIP headers, no torch) drives the C-ABI as the catkin adapter
    does: PCL-mode and GN aligns, VoxelGrid and SegmentDifferences on PointXYZRGB records."""
    import subprocess

    exe = os.path.join(ROOT, "adapter", "cabi_example")
    assert os.path.exists(exe), "build it with `make adapter-example`"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cabi_example: OK" in out.stdout


def test_second_hip_runtime_is_refused():
    """the observed "double free or corruption" with torch's bundled HIP runtime next
    to ROCm's (parallel.py) is now a guard: _lib.load() raises MgicpError when another libamdhip64
    is mapped.  Run in a child process (import torch maps torch/lib/libamdhip64.so)."""
    import subprocess
    import sys

    code = ("import torch, sys; sys.path.insert(0, %r)\n"
            "from leica_point_cloud_processing_amd import _lib\n"
            "try:\n    _lib.load()\nexcept _lib.MgicpError as e:\n    print('REFUSED', e.code)\n"
            "else:\n    print('LOADED')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert "REFUSED -5" in r.stdout, r.stdout + r.stderr
    # and the plain process (no torch) loads it
    code2 = ("import sys; sys.path.insert(0, %r)\nfrom leica_point_cloud_processing_amd import _lib\n"
             "_lib.load(); print('LOADED', sorted(_lib._mapped_hip_runtimes()))\n") % ROOT
    r2 = subprocess.run([sys.executable, "-c", code2], capture_output=True, text=True, timeout=300)
    assert "LOADED" in r2.stdout and "torch" not in r2.stdout, r2.stdout + r2.stderr


@pytest.mark.parametrize("k", [0, 33, -1])
def test_k_out_of_range_is_invalid(k):
    """k_correspondences outside [1, 32] is refused before any device work (include/mi355x_gicp.h)."""
    from leica_point_cloud_processing_amd import _lib

    lib = _lib.load()
    p = _lib.default_params()
    p.k = k
    h = ctypes.c_void_p()
    assert lib.mgicp_create(ctypes.byref(h), ctypes.byref(p)) == _lib.MGICP_E_INVALID

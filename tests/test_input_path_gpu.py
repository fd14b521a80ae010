"""Where every result of the engine starts: the strided host upload (upload_xyz / upload_u32_field and the
pinned ring), pack_points_kernel, the device-pointer setters and xform_points_kernel behind
mgicp_transform_source / mgicp_transform_cloud.  The cases and their premises: tests/input_path_cases.py and
tests/test_input_path_inputs.py.  Every comparison is exact: bit for bit, or integer equality.

  A. the transform calls against synth.transform_points (float32, no FMA, ((T0 x + T1 y) + T2 z) + T3): n at the
     256-thread block edge, in and out strides 12 / 16 / 32 / 48 crossed, in == out, four matrices, the bytes
     outside x, y, z, non-finite / denormal / 1e30 records; mgicp_transform_source after host and device
     set_source at every stride, before and after an align, against the reference and mgicp_transform_cloud.
  B. the upload ring and pack through the identity round trip: set_source then mgicp_transform_source(I) gives
     the coordinates back bit for bit at sizes around the worker split, at the slot edge and one point past
     the ring, at stride 12 (memcpy branch) and 32 (per-record branch); the target through its covariances.
  C. mgicp_set_source_device / mgicp_set_target_device against the host setters: covariances, T, the trace,
     the counts and the fitness bit for bit; the caller's buffer is never written and is copied at call time.
  D. every helper that takes a cloud at strides 16 / 32 / 48 against stride 12; mgicp_voxel_grid's layouts.
  E. the refusals: rgb_offset 0 / 4 / 8, an out stride that is no multiple of 4, the device setters' arguments.

No device pointer reaches the engine unless it lies in a live allocation of device_memory() that holds every
byte the call reads.

As measured on an MI355X: the 58 tests of this module take 2.2 s together.  The slowest are the voxel grid across the colour
slot edge (0.36 s, most of it the oracle and numpy), the target covariances at 699 051 points (0.12 s) and the
2 796 201-point round trips (0.05 s each); every other test stays below 0.1 s.
"""
import ctypes
import functools

import numpy as np
import pytest

import input_path_cases as ic
import param_cases as pc

pytestmark = pytest.mark.gpu

_OF_THE_TEST = []


@pytest.fixture(autouse=True)
def _close_the_tests_engines():
    yield
    while _OF_THE_TEST:
        _OF_THE_TEST.pop().close()


def _engine(**kw):
    from leica_point_cloud_processing_amd.engine import GICPEngine

    e = GICPEngine(**kw)
    _OF_THE_TEST.append(e)
    return e


@pytest.fixture(scope="module")
def eng():
    """one context for the calls that keep nothing between them"""
    from leica_point_cloud_processing_amd.engine import GICPEngine

    e = GICPEngine()
    yield e
    e.close()


def _invalid():
    from leica_point_cloud_processing_amd import _lib

    return _lib.MGICP_E_INVALID


def _cm(T):
    return np.ascontiguousarray(np.asarray(T, np.float32).T).reshape(16)


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _vp(a):
    """a host array's pointer, None for an empty one"""
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


# ------------------------------------------------------------------------------ raw calls, any stride
def _transform_cloud(e, T, inbuf, n, in_stride, outbuf, out_stride):
    return e._lib.mgicp_transform_cloud(e._h, _fp(_cm(T)), _vp(inbuf), n, in_stride, _vp(outbuf), out_stride)


def _transform_source(e, T, outbuf, out_stride):
    return e._lib.mgicp_transform_source(e._h, _fp(_cm(T)), _vp(outbuf), out_stride)


def _set(e, which, buf, n, stride):
    fn = e._lib.mgicp_set_source if which == "source" else e._lib.mgicp_set_target
    e._check(fn(e._h, _vp(buf), n, stride), f"set_{which} at stride {stride}")


def _set_device(e, which, mem, ptr, n, stride):
    """ptr .. ptr + (n - 1) * stride + 12 lies in a live allocation, or nothing is called"""
    assert mem.holds(ptr, (n - 1) * stride + 12)
    (e.set_source_device if which == "source" else e.set_target_device)(ptr, n, stride)


# ------------------------------------------------------------------------------ A. transform calls
def _check_out(outbuf, n, out_stride, want, rest_before, what, floats=False):
    (ic.assert_same_floats if floats else ic.assert_same_bits)(ic.xyz_of(outbuf, n, out_stride), want, what)
    if n and out_stride > 12:
        i = ic.first_difference(ic.rest_of(outbuf, n, out_stride), rest_before)
        assert i is None, f"{what}: byte {12 + i % (out_stride - 12)} of record {i // (out_stride - 12)} was written"


def _transform_cloud_cases(e, p, floats):
    n = len(p)
    for name in ic.MATRICES:
        T = ic.matrix(name)
        want = ic.reference(ic.matrix("general") if name == "last_row" else T, p)
        for si in ic.STRIDES:
            inbuf = ic.records(p, si)
            pristine = inbuf.copy()
            for so in ic.STRIDES:
                what = f"transform_cloud n {n} {name} in {si} out {so}"
                out = np.full(n * so, ic.OUT_FILL, np.uint8)
                assert _transform_cloud(e, T, inbuf, n, si, out, so) == 0, what
                _check_out(out, n, so, want, np.full((n, so - 12), ic.OUT_FILL, np.uint8), what, floats)
                assert ic.first_difference(inbuf, pristine) is None, what + ": the input was written"
            what = f"transform_cloud n {n} {name} in place at {si}"
            assert _transform_cloud(e, T, inbuf, n, si, inbuf, si) == 0, what
            _check_out(inbuf, n, si, want, ic.rest_of(pristine, n, si), what, floats)


@pytest.mark.parametrize("n", ic.XFORM_N)
def test_transform_cloud_strides_matrices_and_untouched_bytes(eng, n):
    _transform_cloud_cases(eng, ic.xform_points(n), floats=False)
    if n == 0:  # nothing is read or written, whatever the pointers
        guard = np.full(48, ic.OUT_FILL, np.uint8)
        assert _transform_cloud(eng, ic.matrix("general"), guard, 0, 48, guard, 48) == 0
        assert (guard == ic.OUT_FILL).all()


def test_transform_cloud_nonfinite_denormal_and_huge_records(eng):
    """every record goes through the float formula: NaN propagates and 0 * Inf = NaN (PCL would skip the
    non-finite records of a non-dense cloud; the engine's contract is the formula)"""
    p = ic.special_points()
    _transform_cloud_cases(eng, p, floats=True)
    out = np.zeros(len(p) * 12, np.uint8)
    assert _transform_cloud(eng, ic.matrix("zero_column"), ic.records(p, 12), len(p), 12, out, 12) == 0
    got = ic.xyz_of(out, len(p), 12)
    assert np.isnan(got[1]).all() and np.isnan(got[0]).all() and np.isfinite(got[10:15]).all()
    out = np.zeros(len(p) * 12, np.uint8)
    assert _transform_cloud(eng, ic.matrix("identity"), ic.records(p, 12), len(p), 12, out, 12) == 0
    ic.assert_same_bits(ic.xyz_of(out, len(p), 12)[10:12], p[10:12], "denormal coordinates through the identity")


def _transform_source_checks(e, p, inbuf, si, when):
    n = len(p)
    for name in ("general", "identity"):
        T = ic.matrix(name)
        want = ic.reference(T, p)
        for so in ic.STRIDES:
            what = f"transform_source n {n} set at {si}, out {so}, {name}, {when}"
            out = np.full(n * so, ic.OUT_FILL, np.uint8)
            assert _transform_source(e, T, out, so) == 0, what
            _check_out(out, n, so, want, np.full((n, so - 12), ic.OUT_FILL, np.uint8), what)
            via_cloud = np.full(n * so, ic.OUT_FILL, np.uint8)
            assert _transform_cloud(e, T, inbuf, n, si, via_cloud, so) == 0, what
            assert ic.first_difference(out, via_cloud) is None, what + ": differs from transform_cloud"


@pytest.mark.parametrize("setter", ["host", "device"])
@pytest.mark.parametrize("n", ic.XFORM_SOURCE_N)
def test_transform_source_after_host_and_device_set_source(n, setter):
    src, tgt = ic.align_pair(n)
    with ic.device_memory() as mem:
        for si in ic.STRIDES:
            inbuf = ic.records(src, si)
            e = _engine()
            if setter == "host":
                _set(e, "source", inbuf, n, si)
            else:
                d = mem.alloc(inbuf.nbytes)
                mem.upload(d, inbuf)
                _set_device(e, "source", mem, d, n, si)
            _transform_source_checks(e, src, inbuf, si, "before any align")
            e.set_target_xyz(tgt)
            T = e.align()
            assert e.last_result["iterations"] >= 1 and np.isfinite(T).all()
            _transform_source_checks(e, src, inbuf, si, "after an align")
            out = np.zeros(n * 12, np.uint8)
            assert _transform_source(e, T, out, 12) == 0
            ic.assert_same_bits(ic.xyz_of(out, n, 12), ic.reference(T, src), f"n {n} set at {si}: the align's T")
            e.close()


# ------------------------------------------------------------------------------ B. upload ring and pack
@pytest.mark.parametrize("stride", ic.RING_STRIDES)
@pytest.mark.parametrize("n", ic.RING_N)
def test_identity_round_trip_through_the_upload_ring(n, stride):
    p = ic.ring_points(n)
    buf = ic.records(p, stride)
    e = _engine()
    _set(e, "source", buf, n, stride)
    del buf
    out = np.zeros(n * 12, np.uint8)
    assert _transform_source(e, ic.matrix("identity"), out, 12) == 0
    e.close()
    ic.assert_same_bits(out.view(np.float32), p, f"source of {n} points uploaded at stride {stride}")


def test_target_through_the_upload_ring_has_the_same_covariances_at_both_strides():
    """the target has no read-back call, so its upload is pinned through what is computed from it: the same
    records set at stride 12 and at stride 32 give the same covariance of every point"""
    n = ic.RING_TARGET_N
    p = ic.ring_points(n)
    src = pc.clouds(2000)[0]
    cov = {}
    for stride in ic.RING_STRIDES:
        e = _engine()
        buf = ic.records(p, stride)
        _set(e, "target", buf, n, stride)
        del buf
        e.set_source_xyz(src)
        cov[stride] = e.debug_covariances("target", n)
        e.close()
    assert np.isfinite(cov[12]).all() and len(np.unique(cov[12][:, 0])) > n // 2
    i = ic.first_difference(cov[12], cov[32])
    assert i is None, f"target covariances differ first at point {i // 6}, entry {i % 6}"


# ------------------------------------------------------------------------------ C. device-pointer setters
def _pair():
    scan, cad, _ = pc.clouds(2000)
    return scan, cad


def _run(e, n_src, n_tgt):
    """everything the issue compares between a host-set and a device-set context"""
    cov_s = e.debug_covariances("source", n_src)
    cov_t = e.debug_covariances("target", n_tgt)
    T = e.align().copy()
    r = e.last_result
    return dict(cov_s=cov_s, cov_t=cov_t, T=T, trace=np.array(e.debug_trace(200), np.float32),
                counts=(r["iterations"], r["n_corr"], r["n_evals"], e.hasConverged()), fitness=e.fitness(T))


def _same_run(a, b, what):
    for f in ("cov_s", "cov_t", "T", "trace"):
        assert a[f].shape == b[f].shape, (what, f)
        i = ic.first_difference(a[f], b[f])
        assert i is None, f"{what}: {f} differs first at flat index {i}"
    assert a["counts"] == b["counts"], (what, a["counts"], b["counts"])
    assert np.float64(a["fitness"]).view(np.uint64) == np.float64(b["fitness"]).view(np.uint64), what


@functools.lru_cache(maxsize=None)
def _host_run():
    scan, cad = _pair()
    e = _engine()
    e.set_source_xyz(scan)
    e.set_target_xyz(cad)
    out = _run(e, len(scan), len(cad))
    e.close()
    assert out["counts"][0] >= 1 and out["counts"][1] > 100 and len(out["trace"]) == out["counts"][0]
    return out


def _device_cloud(mem, xyz, stride, offset):
    """(pointer to the first x, base pointer, the bytes uploaded)"""
    buf, off = ic.device_records(xyz, stride, offset)
    d = mem.alloc(buf.nbytes)
    mem.upload(d, buf)
    return d + off, d, buf


@pytest.mark.parametrize("overwrite", [False, True], ids=["kept", "overwritten_after_set"])
@pytest.mark.parametrize("layout", ic.DEVICE_LAYOUTS, ids=[l[0] for l in ic.DEVICE_LAYOUTS])
def test_device_setters_match_host_setters(layout, overwrite):
    """overwritten_after_set: the buffers are set to 0xff once mgicp_set_*_device has returned -- the engine
    copied them at call time; kept: after the align they hold what was uploaded, byte for byte"""
    _, stride, offset = layout
    scan, cad = _pair()
    with ic.device_memory() as mem:
        ps, ds, bs = _device_cloud(mem, scan, stride, offset)
        pt, dt, bt = _device_cloud(mem, cad, stride, offset)
        if offset:
            assert ps % 16 == 4 and pt % 16 == 4  # float alignment and no more
        e = _engine()
        _set_device(e, "source", mem, ps, len(scan), stride)
        _set_device(e, "target", mem, pt, len(cad), stride)
        if overwrite:
            mem.memset(ds, 0xFF, bs.nbytes)
            mem.memset(dt, 0xFF, bt.nbytes)
        got = _run(e, len(scan), len(cad))
        _same_run(got, _host_run(), f"device clouds at stride {stride} offset {offset}")
        mem.sync()
        if not overwrite:
            assert ic.first_difference(mem.download(ds, bs.nbytes), bs) is None, "the source buffer was written"
            assert ic.first_difference(mem.download(dt, bt.nbytes), bt) is None, "the target buffer was written"
        e.close()


@pytest.mark.parametrize("on_device", ["source", "target"])
def test_one_cloud_from_the_device_and_one_from_the_host(on_device):
    scan, cad = _pair()
    with ic.device_memory() as mem:
        e = _engine()
        for which, xyz in (("source", scan), ("target", cad)):
            if which == on_device:
                p, _, _ = _device_cloud(mem, xyz, 32, 0)
                _set_device(e, which, mem, p, len(xyz), 32)
            else:
                _set(e, which, ic.records(xyz, 32), len(xyz), 32)
        _same_run(_run(e, len(scan), len(cad)), _host_run(), f"{on_device} from the device, the other from the host")
        e.close()


def test_device_setters_refuse_bad_arguments_before_any_launch():
    scan, _ = _pair()
    n = len(scan)
    with ic.device_memory() as mem:
        p, _, _ = _device_cloud(mem, scan, 16, 0)  # n * 16 bytes: every refused call would stay inside it
        e = _engine()
        for fn in (e._lib.mgicp_set_source_device, e._lib.mgicp_set_target_device):
            assert fn(e._h, ctypes.c_void_p(p), 0, 12) == _invalid()
            assert fn(e._h, None, n, 12) == _invalid()
            assert fn(e._h, ctypes.c_void_p(p), n, 8) == _invalid()
            assert fn(e._h, ctypes.c_void_p(p), n, 14) == _invalid()
        # nothing was set: there is no source to transform
        out = np.zeros(16 * n, np.uint8)
        assert _transform_source(e, np.eye(4), out, 16) == _invalid() and not out.any()
        e.close()


# ------------------------------------------------------------------------------ D. strides across the helpers
def _resolution(e, buf, n, stride):
    out = ctypes.c_double()
    e._check(e._lib.mgicp_cloud_resolution(e._h, _vp(buf), n, stride, ctypes.byref(out)), "cloud_resolution")
    return out.value


def _radius_filter(e, buf, n, stride, radius, min_neighbors):
    keep = np.full(n, 7, np.uint8)
    e._check(e._lib.mgicp_radius_filter(e._h, _vp(buf), n, stride, radius, min_neighbors, keep.ctypes.data),
             "radius_filter")
    return keep


def _clusters(e, buf, n, stride, tolerance, min_size):
    from leica_point_cloud_processing_amd import _lib

    labels = np.full(n, -2, np.int32)
    indices = np.full(n, -2, np.int32)
    offsets = np.zeros(n + 1, np.uintp)
    ci = _lib.MgicpClusterInfo()
    e._check(e._lib.mgicp_euclidean_clusters(e._h, _vp(buf), n, stride, tolerance, min_size, 0, labels.ctypes.data,
                                             indices.ctypes.data, offsets.ctypes.data, ctypes.byref(ci)), "clusters")
    m = int(ci.n_clustered_points)
    return labels, indices[:m].copy(), offsets.astype(np.int64), (ci.n_clusters, ci.n_components, m)


def _segdiff(e, T, inbuf, n, in_stride, subbuf, n_sub, sub_stride, thr):
    keep = np.full(n, 7, np.uint8)
    cnt = ctypes.c_size_t()
    tcm = None if T is None else _cm(T)
    e._check(e._lib.mgicp_segment_differences(e._h, None if tcm is None else _fp(tcm), _vp(inbuf), n, in_stride,
                                              _vp(subbuf), n_sub, sub_stride, thr, keep.ctypes.data,
                                              ctypes.byref(cnt)), "segment_differences")
    return keep, int(cnt.value)


def test_resolution_radius_filter_and_clusters_at_every_stride(eng):
    p, bad = ic.helper_cloud()
    n = len(p)
    got = {}
    for stride in ic.STRIDES:
        buf = ic.records(p, stride)
        got[stride] = (_resolution(eng, buf, n, stride),
                       _radius_filter(eng, buf, n, stride, ic.HELPER_RADIUS, 3),
                       _clusters(eng, buf, n, stride, ic.HELPER_TOLERANCE, 2))
    res, keep, (labels, indices, offsets, counts) = got[12]
    # the stride-12 answers are answers: a resolution of the cloud's scale, mixed masks, non-finite records out
    assert 0.005 < res < 0.03, res
    assert set(np.unique(keep)) == {0, 1} and not keep[bad].any() and 0.1 < keep.mean() < 0.9
    assert counts[0] > 50 and (labels[bad] == -1).all() and (labels >= -1).all() and (labels == -1).sum() > 100
    for stride in ic.STRIDES[1:]:
        r, k, (l, i, o, c) = got[stride]
        assert np.float64(r).view(np.uint64) == np.float64(res).view(np.uint64), (stride, r, res)
        assert np.array_equal(k, keep), f"radius filter at stride {stride}"
        assert c == counts and np.array_equal(l, labels) and np.array_equal(i, indices) and np.array_equal(o, offsets), \
            f"clusters at stride {stride}"


@pytest.mark.parametrize("with_T", [False, True], ids=["no_T", "with_T"])
def test_segment_differences_with_independent_strides(eng, with_T):
    """in and sub strides varied independently: swapped stride arguments would read one cloud at the other's"""
    from oracle import ref

    p, bad = ic.helper_cloud()
    q = ic.helper_sub()
    T = ic.helper_T() if with_T else None
    thr = ic.HELPER_SQR_THRESHOLD
    want, want_cnt = ref.segment_differences(ic.reference(T, p) if with_T else p, q, thr)
    assert 0.1 < want.mean() < 0.9 and not want[bad].any()
    for si in ic.STRIDES:
        inbuf = ic.records(p, si)
        for ss in ic.STRIDES:
            keep, cnt = _segdiff(eng, T, inbuf, len(p), si, ic.records(q, ss), len(q), ss, thr)
            assert np.array_equal(keep.astype(bool), want) and set(np.unique(keep)) == {0, 1}, f"in {si} sub {ss}"
            assert cnt == want_cnt, (si, ss, cnt, want_cnt)


def test_set_source_and_set_target_at_every_stride():
    src, tgt = ic.helper_pair()
    got = {}
    for stride in ic.STRIDES:
        e = _engine()
        _set(e, "source", ic.records(src, stride), len(src), stride)
        _set(e, "target", ic.records(tgt, stride), len(tgt), stride)
        got[stride] = _run(e, len(src), len(tgt))
        e.close()
    assert got[12]["counts"][0] >= 1 and got[12]["counts"][1] > len(src) // 2
    for stride in ic.STRIDES[1:]:
        _same_run(got[stride], got[12], f"clouds set at stride {stride} against stride 12")


def _voxel(e, inbuf, n, stride, rgb_offset, leaf, out_stride, min_points=0):
    """(n_out, out buffer of n records, filled with OUT_FILL before the call)"""
    out = np.full(n * out_stride, ic.OUT_FILL, np.uint8)
    nout = ctypes.c_size_t()
    lf = np.full(3, leaf, np.float64)
    rc = e._lib.mgicp_voxel_grid(e._h, _vp(inbuf), n, stride, rgb_offset, lf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                 min_points, _vp(out), out_stride, ctypes.byref(nout))
    return rc, int(nout.value), out


def _voxel_fields(out, m, out_stride, rgb_offset):
    """(xyz, colour words or None) of the first m out records, after checking every other byte of them: zero,
    1.0f at offset 12 where the record has room for it and the colour does not sit there"""
    rows = out[:m * out_stride].reshape(m, out_stride)
    known = np.zeros(out_stride, bool)
    known[:12] = True
    if out_stride >= 16 and rgb_offset != 12:
        assert (rows[:, 12:16].copy().view(np.float32) == 1.0).all(), "1.0f at offset 12"
        known[12:16] = True
    colour = None
    if rgb_offset >= 0:
        colour = rows[:, rgb_offset:rgb_offset + 4].copy().view(np.uint32).reshape(m)
        known[rgb_offset:rgb_offset + 4] = True
    assert not rows[:, ~known].any(), "a byte outside xyz, the 1.0f and the colour is not zero"
    assert (out[m * out_stride:] == ic.OUT_FILL).all(), "records past n_out were written"
    return ic.xyz_of(out, m, out_stride), colour


@functools.lru_cache(maxsize=None)
def _voxel_oracle():
    from leica_point_cloud_processing_amd.cloud import POINT_XYZRGB
    from oracle import ref

    p, _ = ic.helper_cloud()
    rec = ic.colour_records(p, 32, 16).view(POINT_XYZRGB)
    xyz, rgba, ovf = ref.voxel_grid(rec, ic.HELPER_LEAF, 0)
    assert not ovf and 100 < len(xyz) < len(p)
    return xyz, rgba


@pytest.mark.parametrize("layout", ic.VOXEL_LAYOUTS, ids=lambda l: "in%d_rgb%d_out%d" % l)
def test_voxel_grid_layouts(eng, layout):
    stride, rgb_offset, out_stride = layout
    p, _ = ic.helper_cloud()
    n = len(p)
    rc, m, out = _voxel(eng, ic.colour_records(p, stride, rgb_offset), n, stride, rgb_offset, ic.HELPER_LEAF, out_stride)
    assert rc == 0
    xyz, colour = _voxel_fields(out, m, out_stride, rgb_offset)
    rs, ro, rso = ic.VOXEL_REFERENCE_LAYOUT
    rc, mr, outr = _voxel(eng, ic.colour_records(p, rs, ro), n, rs, ro, ic.HELPER_LEAF, rso)
    assert rc == 0 and mr == m
    xyz_r, colour_r = _voxel_fields(outr, mr, rso, ro)
    xyz_o, colour_o = _voxel_oracle()
    assert m == len(xyz_o)
    ic.assert_same_bits(xyz, xyz_r, f"voxel xyz of layout {layout} against {ic.VOXEL_REFERENCE_LAYOUT}")
    ic.assert_same_bits(xyz, xyz_o, f"voxel xyz of layout {layout} against the oracle")
    if rgb_offset >= 0:
        assert np.array_equal(colour, colour_r) and np.array_equal(colour, colour_o), layout
        assert len(np.unique(colour)) > m // 2


def test_voxel_grid_colours_across_the_colour_slot_edge(eng):
    """2 097 153 records: the colour upload's second slot holds the last record's word alone.  The colours
    are a function of the record index, the expected averages integer arithmetic per leaf."""
    from oracle import ref

    p = ic.voxel_big_points()
    n = len(p)
    stride, rgb_offset = 20, 16
    buf = ic.colour_records(p, stride, rgb_offset)
    rc, m, out = _voxel(eng, buf, n, stride, rgb_offset, ic.VOXEL_BIG_LEAF, stride)
    assert rc == 0
    xyz, colour = _voxel_fields(out, m, stride, rgb_offset)
    del out
    idx, want, counts = ic.expected_leaf_colours(p, ic.VOXEL_BIG_LEAF, ic.colour_of(np.arange(n)))
    assert m == len(want) == 513
    # the last record is alone in the last leaf: the second slot's one word comes out as it went in
    assert idx[-1] == idx.max() and counts[-1] == 1 and want[-1] == ic.colour_of(n - 1)
    assert colour[-1] == ic.colour_of(n - 1), f"the last record's colour: {colour[-1]:#010x}"
    bad = np.flatnonzero(colour != want)
    assert not len(bad), f"leaf {bad[0]}: colour {colour[bad[0]]:#010x}, expected {want[bad[0]]:#010x} ({len(bad)} leaves differ)"
    rec = buf.view(np.dtype({"names": ["x", "y", "z", "w", "rgb"], "formats": ["<f4"] * 4 + ["<u4"],
                             "offsets": [0, 4, 8, 12, 16], "itemsize": 20}))
    xyz_o, colour_o, ovf = ref.voxel_grid(rec, ic.VOXEL_BIG_LEAF, 0, rgb_offset=16)
    assert not ovf and np.array_equal(colour_o, want)
    ic.assert_same_bits(xyz, xyz_o, "voxel centroids of 2 097 153 records against the oracle")


# ------------------------------------------------------------------------------ E. refusals
def test_voxel_grid_refuses_a_colour_word_over_xyz(eng):
    p, _ = ic.helper_cloud()
    n = len(p)
    buf = ic.colour_records(p, 32, 16)
    for rgb_offset in (0, 4, 8):
        rc, m, out = _voxel(eng, buf, n, 32, rgb_offset, ic.HELPER_LEAF, 32)
        assert rc == _invalid(), rgb_offset
        assert (out == ic.OUT_FILL).all(), "a refused call wrote its output"
    for rgb_offset in (12, 16, 28):  # every other aligned offset inside the record is taken
        assert _voxel(eng, buf, n, 32, rgb_offset, ic.HELPER_LEAF, 32)[0] == 0, rgb_offset
    assert _voxel(eng, buf, n, 32, 32, ic.HELPER_LEAF, 32)[0] == _invalid()
    assert _voxel(eng, buf, n, 32, 18, ic.HELPER_LEAF, 32)[0] == _invalid()


def test_transform_calls_refuse_a_stride_that_is_no_multiple_of_4():
    src, _ = ic.align_pair(32)
    e = _engine()
    _set(e, "source", ic.records(src, 16), 32, 16)
    out = np.full(32 * 20, ic.OUT_FILL, np.uint8)  # room for 32 records at every stride tried
    for bad in (8, 13, 14, 15, 18):
        assert _transform_source(e, ic.matrix("general"), out, bad) == _invalid(), bad
        assert _transform_cloud(e, ic.matrix("general"), ic.records(src, 16), 32, 16, out, bad) == _invalid(), bad
        assert (out == ic.OUT_FILL).all(), "a refused call wrote its output"
    assert _transform_source(e, ic.matrix("general"), out, 16) == 0
    e.close()

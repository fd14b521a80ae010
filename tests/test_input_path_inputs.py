"""The premises of tests/input_path_cases.py, checked without a GPU: what tests/test_input_path_gpu.py compares
against can tell a wrong kernel from a right one.

  * the transform reference is sensitive to the evaluation order: at the 4099-point case and the general
    matrix a contracted (fused multiply-add) evaluation and a re-associated one each differ from it in at
    least 10 % of the output components (27 % and 25 % as measured), so a kernel built with contraction
    allowed cannot pass the bitwise comparison by luck;
  * the record builder puts x, y, z where the C-ABI reads them and a NaN pattern everywhere else, so that a
    read with a wrong stride or offset meets NaN;
  * the sizes of the ring cases sit where the issue's reasoning puts them: at the slot edge and one point
    past the ring;
  * the helper cloud makes every helper's output a mixed one (a constant answer would pass any comparison).
"""
import numpy as np
import pytest

import input_path_cases as ic


def _differs(a, b):
    return float(np.mean(a.view(np.uint32) != b.view(np.uint32)))


def test_reference_tells_a_contracted_and_a_reassociated_evaluation_apart():
    T, p = ic.matrix("general"), ic.xform_points(4099)
    ref = ic.reference(T, p)
    fused, reassoc = _differs(ic.contracted(T, p), ref), _differs(ic.reassociated(T, p), ref)
    print(f"components that differ from the reference: contracted {fused:.3f}, re-associated {reassoc:.3f}")
    assert fused >= 0.10, fused
    assert reassoc >= 0.10, reassoc
    # and the reference is what it says: float64 agrees with it to float rounding, so all three are the same sum
    exact = p.astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
    for v in (ref, ic.contracted(T, p), ic.reassociated(T, p)):
        assert np.abs(v - exact).max() < 4 * 2.0 ** -23


def test_matrices():
    g = ic.matrix("general")
    assert np.abs(g[:3, :3] @ g[:3, :3].T - np.eye(3)).max() < 1e-6 and not np.array_equal(g, np.eye(4))
    assert np.array_equal(ic.matrix("identity"), np.eye(4, dtype=np.float32))
    lr = ic.matrix("last_row")
    assert np.array_equal(lr[:3], g[:3]) and lr[3].tolist() == [5, 6, 7, 8]
    zc = ic.matrix("zero_column")
    assert not zc[:, 1].any() and zc[:3, [0, 2, 3]].all()
    p = ic.xform_points(257)
    assert np.array_equal(ic.reference(lr, p), ic.reference(g, p))
    # the identity gives back finite records without -0 bit for bit
    r = ic.ring_points(65)
    assert ic.first_difference(ic.reference(ic.matrix("identity"), r), r) is None
    assert r.min() >= 0.25 and r.max() < 1.0


def test_special_points_reference():
    """NaN propagates, 0 * Inf is NaN, denormal and 1e30 coordinates stay representable"""
    p = ic.special_points()
    assert len(p) == 257
    bad = ~np.isfinite(p).all(axis=1)
    assert bad.sum() == 8 and bad[0] and bad[256] and bad[255]
    assert (~np.isfinite(p)).sum(axis=1).max() == 1  # one coordinate of a record
    ref = ic.reference(ic.matrix("general"), p)
    assert np.isnan(ref[0]).all() and np.isnan(ref[3]).all()  # a NaN coordinate reaches x, y and z
    assert not np.isfinite(ref[bad]).any()
    zc = ic.reference(ic.matrix("zero_column"), p)
    assert np.isnan(zc[1]).all()        # y = +Inf against a zero column: 0 * Inf
    assert np.isinf(ic.reference(ic.matrix("general"), p)[1]).all()
    assert np.isfinite(zc[~bad]).all() and np.isfinite(ref[~bad]).all()
    tiny = np.abs(p[10])
    assert (tiny > 0).all() and (tiny < np.finfo(np.float32).tiny).all()
    assert (ref[10] == ic.matrix("general")[:3, 3]).all()  # a denormal sum vanishes beside the translation
    ident = ic.reference(ic.matrix("identity"), p)
    assert ic.first_difference(ident[10:12], p[10:12]) is None  # and survives where nothing is added to it
    assert np.abs(ref[12]).max() > 1e29 and np.isfinite(ref[12:15]).all()


@pytest.mark.parametrize("stride", ic.STRIDES)
def test_records_layout_and_poison(stride):
    p = ic.xform_points(257)
    buf = ic.records(p, stride)
    assert buf.dtype == np.uint8 and buf.nbytes == 257 * stride and buf.ctypes.data % 4 == 0
    assert ic.first_difference(ic.xyz_of(buf, 257, stride), p) is None
    rest = ic.rest_of(buf, 257, stride)
    assert rest.shape == (257, stride - 12)
    if stride > 12:
        assert (rest.reshape(-1).view(np.uint32) == ic.POISON).all()
        assert np.isnan(rest.reshape(-1).view(np.float32)).all()
        # read with another stride, or one word off, the records hold NaN
        for wrong in ic.STRIDES:
            if wrong != stride and wrong < stride:
                assert np.isnan(ic.xyz_of(buf, 257, wrong)).any()
        assert np.isnan(ic.xyz_of(buf[4:], 256, stride)).any(axis=1).all()


def test_device_layouts():
    p = ic.xform_points(257)
    for name, stride, off in ic.DEVICE_LAYOUTS:
        buf, first = ic.device_records(p, stride, off)
        assert buf.nbytes == 257 * stride and first == off, name
        assert ic.first_difference(ic.xyz_of(buf, 257, stride, lead=off), p) is None, name
        assert off + 256 * stride + 12 <= buf.nbytes  # the last z ends inside the buffer
    assert [(s, o) for _, s, o in ic.DEVICE_LAYOUTS] == [(12, 0), (16, 0), (32, 0), (16, 4)]


def test_ring_sizes():
    assert ic.SLOT_POINTS == 699_050 and ic.RING_POINTS == 2_796_200 and ic.SLOT_COLOURS == 2_097_152
    assert ic.SLOT_POINTS * 12 <= ic.SLOT_BYTES < (ic.SLOT_POINTS + 1) * 12
    assert set(ic.RING_N) == {32, 63, 64, 65, 699_049, 699_050, 699_051, 2_796_201}
    chunks = lambda n: -(-n // ic.SLOT_POINTS)  # noqa: E731
    assert [chunks(n) for n in (699_049, 699_050, 699_051)] == [1, 1, 2]
    assert chunks(ic.RING_POINTS) == ic.RING_SLOTS and chunks(ic.RING_POINTS + 1) == ic.RING_SLOTS + 1
    assert ic.VOXEL_BIG_N == 2_097_153 and ic.RING_TARGET_N == 699_051
    # the cnt * part / parts split: for any number of parts the ranges tile [0, cnt) with no gap or overlap
    for cnt in (32, 63, 64, 65):
        for parts in (4, 64, 96, 256):
            edges = [cnt * q // parts for q in range(parts + 1)]
            assert edges[0] == 0 and edges[-1] == cnt and all(a <= b for a, b in zip(edges, edges[1:]))
    assert ic.first_difference(np.arange(10.0), np.arange(10.0)) is None
    a = np.zeros(1_000_000, np.float32)
    b = a.copy()
    b[777_777] = 1
    b[900_000] = 1
    assert ic.first_difference(a, b) == 777_777
    with pytest.raises(AssertionError, match="flat index 777777"):
        ic.assert_same_bits(a, b, "x")
    nan2 = np.array([np.nan, 1.0], np.float32)
    ic.assert_same_floats(nan2, nan2.copy(), "x")
    with pytest.raises(AssertionError):
        ic.assert_same_floats(nan2, np.array([1.0, np.nan], np.float32), "x")


def test_helper_cloud_gives_mixed_answers():
    p, bad = ic.helper_cloud()
    assert len(p) == ic.HELPER_N and len(bad) == ic.HELPER_BAD == (~np.isfinite(p).all(axis=1)).sum()
    assert bad[0] == 0 and bad[-1] == ic.HELPER_N - 1
    fin = np.isfinite(p).all(axis=1)
    d2 = ic.brute_d2(p, p[fin])
    with np.errstate(invalid="ignore"):
        near = (d2 < np.float32(ic.HELPER_RADIUS ** 2)).sum(axis=1)
        links = (d2 < np.float32(ic.HELPER_TOLERANCE ** 2)).sum(axis=1)
    keep = fin & (near >= 3)
    assert 0.1 < keep[fin].mean() < 0.9, keep.mean()           # the radius filter's mask
    assert 0.2 < (links[fin] >= 2).mean() < 0.9                # clustering: linked and single records
    q = ic.helper_sub()
    assert (~np.isfinite(q).all(axis=1)).sum() == 5
    qf = q[np.isfinite(q).all(axis=1)]
    for T in (None, ic.helper_T()):
        moved = p if T is None else ic.reference(T, p)
        with np.errstate(invalid="ignore"):
            d2 = ic.brute_d2(moved, qf)
            far = fin & (np.where(np.isnan(d2), np.inf, d2).min(axis=1) > np.float32(ic.HELPER_SQR_THRESHOLD))
        assert 0.1 < far[fin].mean() < 0.9, far.mean()         # the segment differences' mask
    src, tgt = ic.helper_pair()
    assert len(src) == len(tgt) == ic.HELPER_N - ic.HELPER_BAD and np.isfinite(src).all() and np.isfinite(tgt).all()


def test_voxel_cases():
    assert ic.VOXEL_REFERENCE_LAYOUT in ic.VOXEL_LAYOUTS
    for stride, rgb, out in ic.VOXEL_LAYOUTS:
        assert rgb == -1 or (12 <= rgb and rgb + 4 <= min(stride, out) and rgb % 4 == 0)
    p, _ = ic.helper_cloud()
    buf = ic.colour_records(p, 48, 44)
    rows = buf.reshape(-1, 48)
    assert np.array_equal(rows[:, 44:48].copy().view(np.uint32).reshape(-1), ic.colour_of(np.arange(len(p))))
    assert (rows[:, 12:44].copy().view(np.uint32) == ic.POISON).all()
    c = ic.colour_of(np.arange(1 << 16))
    for shift in (0, 8, 16, 24):
        assert len(np.unique((c >> np.uint32(shift)) & np.uint32(0xFF))) == 256
    # the integer colour rule against a direct evaluation, on a small cloud
    fin = p[np.isfinite(p).all(axis=1)]
    idx, word, counts = ic.expected_leaf_colours(fin, ic.HELPER_LEAF, ic.colour_of(np.arange(len(fin))))
    assert len(word) == len(counts) > 100 and counts.sum() == len(fin)
    leaf0 = np.flatnonzero(idx == np.unique(idx)[0])
    ch = (ic.colour_of(leaf0) >> np.uint32(8)) & np.uint32(0xFF)
    assert (int(word[0]) >> 8) & 0xFF == int(np.float32(ch.astype(np.float32).sum()) / np.float32(len(leaf0)))


def test_voxel_case_across_the_colour_slot_edge_against_the_oracle():
    """the integer colour rule is the oracle's float one at this case, and the record past the slot edge is
    alone in its leaf"""
    from oracle import ref

    p = ic.voxel_big_points()
    n = len(p)
    assert n == ic.SLOT_COLOURS + 1 and np.isfinite(p).all()
    idx, word, counts = ic.expected_leaf_colours(p, ic.VOXEL_BIG_LEAF, ic.colour_of(np.arange(n)))
    assert len(word) == 513 and counts[-1] == 1 and idx[-1] == idx.max() and word[-1] == ic.colour_of(n - 1)
    assert counts[:-1].min() > 3500 and counts.max() < 4700
    rec = ic.colour_records(p, 20, 16).view(np.dtype({"names": ["x", "y", "z", "w", "rgb"], "formats": ["<f4"] * 4 + ["<u4"],
                                                      "offsets": [0, 4, 8, 12, 16], "itemsize": 20}))
    xyz, rgba, ovf = ref.voxel_grid(rec, ic.VOXEL_BIG_LEAF, 0, rgb_offset=16)
    assert not ovf and len(xyz) == 513
    assert np.array_equal(rgba, word)

"""The cases of the input-path tests: where every result of the engine starts.

Shared by tests/test_input_path_inputs.py (CPU: the premises of the cases) and tests/test_input_path_gpu.py
(the strided host upload, pack_points_kernel, the device-pointer setters and xform_points_kernel behind
mgicp_transform_source / mgicp_transform_cloud).  Nothing here calls the engine; device_memory() talks to the
HIP runtime the engine's library has mapped, never to a second one.  Every cloud is seeded, cached, made once
per process and read-only.

Record buffers: records(xyz, stride) lays n points out as the C-ABI takes them, x, y, z at bytes 0/4/8 of
records of `stride` bytes.  Every other byte holds POISON, a NaN bit pattern, so a read at a wrong offset or
with a wrong stride shows in whatever is computed from it.

The upload ring (csrc/host_upload.hpp): 4 pinned slots of 8 MiB.  One slot carries SLOT_POINTS = 699 050 xyz
triples, the ring RING_POINTS = 2 796 200; past that a slot is reused after an event wait.  The colour upload of
mgicp_voxel_grid fills a slot with SLOT_COLOURS = 2 097 152 words.
"""
import contextlib
import ctypes
import functools

import numpy as np

SLOT_BYTES = 8 << 20
RING_SLOTS = 4
SLOT_POINTS = SLOT_BYTES // 12   # 699 050
RING_POINTS = RING_SLOTS * SLOT_POINTS  # 2 796 200
SLOT_COLOURS = SLOT_BYTES // 4   # 2 097 152
POISON = 0x7FC0DEAD              # a quiet NaN as a float; no byte of it is 0x00, 0xff or that of a 1.0f

STRIDES = (12, 16, 32, 48)

# ------------------------------------------------------------------------------ A. transform calls
XFORM_N = (0, 1, 2, 3, 255, 256, 257, 4099)      # mgicp_transform_cloud; 256 threads per block
XFORM_SOURCE_N = (32, 255, 256, 257, 4099)       # mgicp_transform_source; never below k = 32
MATRICES = ("general", "identity", "last_row", "zero_column")
OUT_FILL = 0xA5                                   # the out records before a call


def records(xyz, stride, lead=0, tail=0):
    """uint8 buffer of lead + n * stride + tail bytes: x, y, z at bytes 0/4/8 of record i, which starts at
    lead + i * stride; every other 4-byte word is POISON (lead, stride, tail: multiples of 4)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    assert stride >= 12 and stride % 4 == 0 and lead % 4 == 0 and tail % 4 == 0
    buf = np.full((lead + n * stride + tail) // 4, POISON, np.uint32).view(np.uint8)
    if n:
        buf[lead:lead + n * stride].reshape(n, stride)[:, :12] = xyz.view(np.uint8).reshape(n, 12)
    return buf


def xyz_of(buf, n, stride, lead=0):
    """(n, 3) float32 copy of the x, y, z of n records"""
    if n == 0:
        return np.zeros((0, 3), np.float32)
    buf = np.asarray(buf, np.uint8)
    assert lead + (n - 1) * stride + 12 <= buf.nbytes
    rows = np.lib.stride_tricks.as_strided(buf[lead:], shape=(n, 12), strides=(stride, 1), writeable=False)
    return np.ascontiguousarray(rows).view(np.float32).reshape(n, 3).copy()


def rest_of(buf, n, stride):
    """the bytes of n records outside their x, y, z: (n, stride - 12) uint8 copy"""
    return np.asarray(buf, np.uint8)[:n * stride].reshape(n, stride)[:, 12:].copy()


def first_difference(a, b, chunk=1 << 18):
    """index of the first element at which two equally shaped arrays differ bit for bit, None if none does;
    compared chunk by chunk, so that a mismatch in millions of values costs one small report"""
    a = np.ascontiguousarray(a).reshape(-1)
    b = np.ascontiguousarray(b).reshape(-1)
    assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize, (a.shape, b.shape)
    ua = a.view(f"u{a.dtype.itemsize}")
    ub = b.view(f"u{b.dtype.itemsize}")
    for s in range(0, len(ua), chunk):
        ne = ua[s:s + chunk] != ub[s:s + chunk]
        if ne.any():
            return s + int(np.argmax(ne))
    return None


def assert_same_bits(got, want, what):
    """bitwise equality, reported as the first differing flat index and the two values there"""
    i = first_difference(got, want)
    if i is not None:
        g, w = np.asarray(got).reshape(-1)[i], np.asarray(want).reshape(-1)[i]
        raise AssertionError(f"{what}: first difference at flat index {i} (component {i % 3} of record {i // 3} "
                             f"for xyz): got {g!r}, want {w!r}")


def assert_same_floats(got, want, what):
    """the rule for outputs that may hold NaN: the same NaN positions, and every other value bit for bit (a
    NaN's payload is not pinned)"""
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), (what, "NaN positions differ", np.argwhere(ng != nw)[:5].tolist())
    assert_same_bits(np.where(ng, np.float32(0), got), np.where(nw, np.float32(0), want), what)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """float32 4 x 4, read-only.  "last_row" is "general" with the last row (5, 6, 7, 8): the calls read the
    3 x 4 alone, so its result is that of "general".  "zero_column" has a zero second column: y drops out of
    every finite record, and an infinite y gives 0 * Inf = NaN."""
    from leica_point_cloud_processing_amd import synth

    T = synth.axis_angle_matrix([1, 2, 3], 0.7, t=(0.1, -0.2, 0.3)).astype(np.float32)
    if name == "identity":
        T = np.eye(4, dtype=np.float32)
    elif name == "last_row":
        T[3] = [5, 6, 7, 8]
    elif name == "zero_column":
        T[:, 1] = 0
    else:
        assert name == "general", name
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def xform_points(n):
    """n seeded float32 points, uniform in (-1, 1), read-only"""
    g = np.random.Generator(np.random.PCG64(7000 + n))
    p = g.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def special_points():
    """257 records (two blocks): xform_points(257) with NaN, +Inf and -Inf in one coordinate of some records
    (each of x, y, z; the first and the last record and both sides of the block edge among them), denormal
    coordinates and coordinates at 1e30"""
    p = xform_points(257).copy()
    p[0, 0] = np.nan
    p[1, 1] = np.inf
    p[2, 2] = -np.inf
    p[3, 1] = np.nan
    p[4, 0] = -np.inf
    p[5, 2] = np.inf
    p[255, 2] = np.nan
    p[256, 0] = np.inf
    p[10] = [1e-40, -3e-42, 1.4e-45]              # denormals: every product with a rotation entry is one too
    p[11] = [1e-39, 0.5, -1e-41]
    p[12] = [1e30, -1e30, 1e30]
    p[13] = [1e30, 0.25, -2.0]
    p[14] = [0.0, -0.0, 1e30]
    p.setflags(write=False)
    return p


def reference(T, xyz):
    """pcl::transformPointCloud's xyz: synth.transform_points, float32, ((T00 x + T01 y) + T02 z) + T03"""
    from leica_point_cloud_processing_amd import synth

    with np.errstate(invalid="ignore", over="ignore"):
        return synth.transform_points(np.asarray(T, np.float32), np.asarray(xyz, np.float32).reshape(-1, 3))


def contracted(T, xyz):
    """the same sum as a compiler allowed to contract would evaluate it: a = T0 x, a = fma(T1, y, a),
    a = fma(T2, z, a), a + T3.  The fma is emulated in float64, where the product of two floats is exact."""
    T = np.asarray(T, np.float32)
    p = np.asarray(xyz, np.float32).astype(np.float64)
    out = np.empty((len(p), 3), np.float32)
    for r in range(3):
        t = T[r].astype(np.float64)
        a = (t[0] * p[:, 0]).astype(np.float32)
        a = (t[1] * p[:, 1] + a.astype(np.float64)).astype(np.float32)
        a = (t[2] * p[:, 2] + a.astype(np.float64)).astype(np.float32)
        out[:, r] = a + T[r, 3]
    return out


def reassociated(T, xyz):
    """the float32 products summed as (x + (y + z)) + t"""
    T = np.asarray(T, np.float32)
    p = np.asarray(xyz, np.float32)
    out = np.empty((len(p), 3), np.float32)
    for r in range(3):
        out[:, r] = (T[r, 0] * p[:, 0] + (T[r, 1] * p[:, 1] + T[r, 2] * p[:, 2])) + T[r, 3]
    return out


@functools.lru_cache(maxsize=None)
def align_pair(n):
    """(source, target) of n points each for the align between two mgicp_transform_source calls: the source
    fills a 10 cm cube; the target is the source turned by 0.02 rad about z through the cube's centre and
    shifted by 1 mm, so every point has its partner far inside the 4 cm gate."""
    g = np.random.Generator(np.random.PCG64(7100 + n))
    src = np.array([1.0, 2.0, 0.5]) + g.uniform(0.0, 0.1, (n, 3))
    c, s = np.cos(0.02), np.sin(0.02)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    ctr = np.array([1.05, 2.05, 0.55])
    tgt = (src - ctr) @ R.T + ctr + np.array([1e-3, -5e-4, 5e-4])
    out = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------ B. upload ring
# the cnt * part / parts split of one slot (parts = 4 x the host threads) at sizes around it, the slot edge,
# and one point past the ring: the fifth chunk reuses slot 0 after its event
RING_N = (32, 63, 64, 65, SLOT_POINTS - 1, SLOT_POINTS, SLOT_POINTS + 1, RING_POINTS + 1)
RING_STRIDES = (12, 32)  # the memcpy branch and the per-record branch of upload_xyz
RING_TARGET_N = SLOT_POINTS + 1


@functools.lru_cache(maxsize=2)
def ring_points(n):
    """n seeded float32 points in [0.25, 1): finite, no -0, so the identity gives them back bit for bit"""
    g = np.random.Generator(np.random.PCG64(7200))
    p = g.random((n, 3), np.float32) * np.float32(0.75) + np.float32(0.25)
    p.setflags(write=False)
    return p


# ------------------------------------------------------------------------------ C. device-pointer setters
# (name, stride, byte offset of x in the record): the last has its xyz 4 bytes into 16-byte records, a
# pointer with float alignment and no more
DEVICE_LAYOUTS = (("s12", 12, 0), ("s16", 16, 0), ("s32", 32, 0), ("s16_off4", 16, 4))


def device_records(xyz, stride, offset):
    """(buffer, byte offset of the first x): n * stride bytes whose record i holds x, y, z at
    offset + i * stride; the last record's z ends inside the buffer"""
    assert offset + 12 <= stride
    n = len(xyz)
    buf = records(xyz, stride, lead=offset)[:n * stride]
    return np.ascontiguousarray(buf), offset


@contextlib.contextmanager
def device_memory():
    """hipMalloc / hipMemcpy / hipMemset of the HIP runtime that libmgicp.so has mapped (opened again by its
    path: no second runtime, no torch); every allocation is freed on exit.  Yields an object with
    alloc(nbytes) -> int pointer, upload(ptr, uint8 array), download(ptr, nbytes) -> uint8 array,
    memset(ptr, byte, nbytes), sync()."""
    from leica_point_cloud_processing_amd import _lib

    _lib.load()
    paths = _lib._mapped_hip_runtimes()
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(next(iter(paths)))
    P, SZ = ctypes.c_void_p, ctypes.c_size_t
    hip.hipMalloc.argtypes, hip.hipMalloc.restype = [ctypes.POINTER(P), SZ], ctypes.c_int
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [P, P, SZ, ctypes.c_int], ctypes.c_int
    hip.hipMemset.argtypes, hip.hipMemset.restype = [P, ctypes.c_int, SZ], ctypes.c_int
    hip.hipFree.argtypes, hip.hipFree.restype = [P], ctypes.c_int
    hip.hipDeviceSynchronize.argtypes, hip.hipDeviceSynchronize.restype = [], ctypes.c_int

    def ck(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: HIP status {rc}")

    class Mem:
        def __init__(self):
            self.live = {}

        def alloc(self, nbytes):
            p = P()
            ck(hip.hipMalloc(ctypes.byref(p), nbytes), "hipMalloc")
            self.live[p.value] = nbytes
            return p.value

        def _inside(self, ptr, nbytes):
            assert any(b <= ptr and ptr + nbytes <= b + sz for b, sz in self.live.items()), "outside every allocation"

        def upload(self, ptr, data):
            data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            self._inside(ptr, data.nbytes)
            ck(hip.hipMemcpy(ptr, data.ctypes.data, data.nbytes, 1), "hipMemcpy to the device")

        def download(self, ptr, nbytes):
            self._inside(ptr, nbytes)
            out = np.empty(nbytes, np.uint8)
            ck(hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2), "hipMemcpy to the host")
            return out

        def memset(self, ptr, byte, nbytes):
            self._inside(ptr, nbytes)
            ck(hip.hipMemset(ptr, byte, nbytes), "hipMemset")
            self.sync()

        def sync(self):
            ck(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")

        def holds(self, ptr, nbytes):
            """the whole of [ptr, ptr + nbytes) lies in one live allocation"""
            self._inside(ptr, nbytes)
            return True

    m = Mem()
    try:
        yield m
    finally:
        hip.hipDeviceSynchronize()
        for p in list(m.live):
            del m.live[p]
            ck(hip.hipFree(p), "hipFree")


# ------------------------------------------------------------------------------ D. strides across the helpers
HELPER_N = 3000
HELPER_BAD = 20
HELPER_RADIUS = 0.02      # radius filter: about 3.7 points expected in the ball, the self included
HELPER_TOLERANCE = 0.015  # clustering
HELPER_SQR_THRESHOLD = 1e-4
HELPER_LEAF = 0.05


def _with_bad(p, g, nbad):
    """nbad records of p with NaN, +Inf or -Inf in one coordinate, the first and the last record among them"""
    idx = np.concatenate([[0, len(p) - 1], g.choice(np.arange(1, len(p) - 1), nbad - 2, replace=False)])
    for j, i in enumerate(idx):
        p[i, j % 3] = (np.nan, np.inf, -np.inf)[(j // 3) % 3]
    return np.sort(idx)


@functools.lru_cache(maxsize=None)
def helper_cloud():
    """(xyz, indices of the non-finite records): HELPER_N seeded points in a 30 cm cube, HELPER_BAD of them
    non-finite"""
    g = np.random.Generator(np.random.PCG64(7300))
    p = (np.array([1.0, 2.0, 0.5]) + g.uniform(0.0, 0.3, (HELPER_N, 3))).astype(np.float32)
    bad = _with_bad(p, g, HELPER_BAD)
    p.setflags(write=False)
    bad.setflags(write=False)
    return p, bad


@functools.lru_cache(maxsize=None)
def helper_sub():
    """the cloud that mgicp_segment_differences subtracts: every second finite record of helper_cloud() moved
    by up to 4 mm per axis, plus 5 non-finite records"""
    g = np.random.Generator(np.random.PCG64(7301))
    p, bad = helper_cloud()
    keep = np.setdiff1d(np.arange(HELPER_N), bad)[::2]
    q = (p[keep] + g.uniform(-4e-3, 4e-3, (len(keep), 3))).astype(np.float32)
    _with_bad(q, g, 5)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def helper_T():
    """the transform mgicp_segment_differences applies to its input: 0.01 rad about the cube's centre, 1 mm"""
    from leica_point_cloud_processing_amd import synth

    T = synth.axis_angle_matrix([0, 0, 1], 0.01, center=(1.15, 2.15, 0.65), t=(1e-3, 0.0, -1e-3)).astype(np.float32)
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def helper_pair():
    """(source, target) for set_source / set_target at every stride: the finite records of helper_cloud(), and
    those moved by helper_T() with 0.1 mm of seeded noise"""
    g = np.random.Generator(np.random.PCG64(7302))
    p, bad = helper_cloud()
    src = np.ascontiguousarray(np.delete(p, bad, axis=0))
    tgt = (reference(helper_T(), src).astype(np.float64) + g.normal(0.0, 1e-4, src.shape)).astype(np.float32)
    for a in (src, tgt):
        a.setflags(write=False)
    return src, tgt


def brute_d2(a, b):
    """float32 squared distances ((dx^2) + dy^2) + dz^2 between every record of a and of b, (len(a), len(b));
    non-finite records give NaN or Inf"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = a[:, None, :] - b[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# mgicp_voxel_grid: (in stride, rgb_offset, out stride); the second is the layout of pcl::PointXYZRGB, the
# layout of the oracle's records
VOXEL_LAYOUTS = ((12, -1, 12), (20, 16, 20), (32, 16, 32), (48, 44, 48))
VOXEL_REFERENCE_LAYOUT = (32, 16, 32)
VOXEL_BIG_N = SLOT_COLOURS + 1  # the colour upload's second slot holds one word
VOXEL_BIG_LEAF = 0.25


def colour_of(index):
    """the colour word of record `index`: a function of the index alone, every byte of it varying"""
    return ((np.asarray(index, np.uint64) * np.uint64(2654435761) + np.uint64(0x01020304)) & np.uint64(0xFFFFFFFF)
            ).astype(np.uint32)


def colour_records(xyz, stride, rgb_offset):
    """records(xyz, stride) with colour_of(i) at rgb_offset of record i (-1: no colour)"""
    n = len(xyz)
    buf = records(xyz, stride)
    if rgb_offset >= 0:
        assert rgb_offset >= 12 and rgb_offset + 4 <= stride
        buf.reshape(n, stride)[:, rgb_offset:rgb_offset + 4] = colour_of(np.arange(n)).view(np.uint8).reshape(n, 4)
    return buf


@functools.lru_cache(maxsize=1)
def voxel_big_points():
    """VOXEL_BIG_N seeded float32 points in [0, 2)^3: 512 leaves of edge 0.25, about 4096 records each; the
    last record, the one word of the colour upload's second slot, sits alone in a 513th leaf, so that its
    colour comes out as it went in (among 4096 others it would hardly move an average)"""
    g = np.random.Generator(np.random.PCG64(7400))
    p = g.random((VOXEL_BIG_N, 3), np.float32) * np.float32(2.0)
    p[-1] = 2.125
    p.setflags(write=False)
    return p


def expected_leaf_colours(xyz, leaf, colours):
    """(leaf index of every record, colour word of every occupied leaf in ascending leaf index) for finite xyz,
    with VoxelGrid's own float arithmetic for the index (floor(p * (1.0f / leaf)) less the floor of the
    minimum) and integer arithmetic for the colour: each of b, g, r, a is floor(sum / count).  The engine sums
    the channels as floats and truncates the float quotient; that is the same number while count * 255 < 2^24
    (the sums are exact) and count < 2^17 (a quotient that is no integer lies at least 1 / count from one, and
    half an ulp below 256 is 2^-17), which the caller asserts."""
    xyz = np.asarray(xyz, np.float32)
    inv = np.float32(1.0) / np.float32(leaf)
    cell = np.floor(xyz * inv)
    lo = np.floor(xyz.min(axis=0) * inv)
    hi = np.floor(xyz.max(axis=0) * inv)
    div = (hi - lo + 1).astype(np.int64)
    ijk = (cell - lo).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    leaves, inverse, counts = np.unique(idx, return_inverse=True, return_counts=True)
    assert counts.max() * 255 < 2 ** 24 and counts.max() < 2 ** 17, counts.max()
    word = np.zeros(len(leaves), np.uint32)
    c = np.asarray(colours, np.uint32)
    for shift in (0, 8, 16, 24):
        s = np.bincount(inverse, weights=((c >> np.uint32(shift)) & np.uint32(0xFF)).astype(np.float64),
                        minlength=len(leaves)).astype(np.int64)
        word |= (s // counts).astype(np.uint32) << np.uint32(shift)
    return idx, word, counts

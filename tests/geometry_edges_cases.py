"""Clouds, transforms and float32 brute-force references of the geometry-edge tests.

Shared by tests/test_geometry_edges_inputs.py (CPU: the inputs are what they claim, checked on the
oracle alone) and tests/test_geometry_edges_gpu.py (engine vs oracle).  Nothing here touches the
engine.  Every builder is cached: a cloud is made once per process and must not be modified.
"""
import functools
import math

import numpy as np

# ------------------------------------------------------------------------------- family 1
OFFSETS = {
    "origin": (0.0, 0.0, 0.0),
    "site300": (300.25, -150.5, 75.125),
    "site4096": (4096.5, -2048.25, 1024.75),
}
PAIRS = ("part", "patch")
# the patch pair's gate: the target (every other patch point, 4000 points on 0.2 m x 0.2 m) has a
# density of 1e5 points / m^2, so a source point without an exact partner finds a target point within r
# with probability 1 - exp(-1e5 pi r^2) -- one half at r = 1.5 mm.  At T = I the 4000 exact partners are
# accepted as well (~3/4 in all), after a few-millimetre shift nobody has a partner (~1/2)
PATCH_GATE = 1.5e-3
PART_GATE = 0.04  # the engine's and PCL's default
SHIFT = (0.002, -0.0015, 0.0005)  # the few-millimetre shift of the sweeps
ROT_ANGLE = 0.3
PART_AXIS = (0.3, 0.5, 0.81)
FDF_STATES = (
    (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    (0.002, -0.0015, 0.0005, 0.0, 0.0, 0.0),
    (0.001, -0.002, 0.0005, 0.0003, -0.0002, 0.0004),
)


@functools.lru_cache(maxsize=None)
def part6000():
    from leica_point_cloud_processing_amd import synth

    return synth.scan_vs_cad(6000, 6000)


@functools.lru_cache(maxsize=None)
def patch8000():
    """dense patch: x, y uniform in [0, 0.2] m, z ~ N(0, 3e-4) -- ~1.6 mm spacing"""
    rng = np.random.default_rng(5)
    p = np.empty((8000, 3), np.float64)
    p[:, 0] = rng.uniform(0.0, 0.2, 8000)
    p[:, 1] = rng.uniform(0.0, 0.2, 8000)
    p[:, 2] = rng.normal(0.0, 3e-4, 8000)
    return p.astype(np.float32)


def shifted(xyz, off):
    """xyz + off, in float32"""
    return np.ascontiguousarray(np.asarray(xyz, np.float32) + np.asarray(off, np.float32), np.float32)


@functools.lru_cache(maxsize=None)
def far_pair(pair: str, offset: str):
    """(source, target, gate) of family 1: the pair moved by the offset, both clouds, in float32"""
    off = OFFSETS[offset]
    if pair == "part":
        src, cad, _ = part6000()
        return shifted(src, off), shifted(cad, off), PART_GATE
    p = patch8000()
    return shifted(p, off), shifted(p[::2], off), PATCH_GATE


def translation(t) -> np.ndarray:
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = t
    return T


@functools.lru_cache(maxsize=None)
def far_transforms(pair: str, offset: str):
    """[identity, the few-millimetre shift, a 0.3 rad rotation about the source's own centre] as float32
    4x4.  The rotation is composed about the cloud's centre (about the origin it would fling a site-frame
    cloud a kilometre away), so the moved source still overlaps the target: the patch turns in its own
    plane, the part about its usual axis."""
    from leica_point_cloud_processing_amd import synth

    src, _, _ = far_pair(pair, offset)
    c = src.astype(np.float64).mean(0)
    axis = PART_AXIS if pair == "part" else (0.0, 0.0, 1.0)
    R = synth.axis_angle_matrix(axis, ROT_ANGLE, c).astype(np.float32)
    return [np.eye(4, dtype=np.float32), translation(SHIFT), R]


def segment_threshold(pair: str) -> float:
    """squared threshold near the squared point spacing of the pair's target"""
    return 0.03 ** 2 if pair == "part" else 0.0016 ** 2


# ------------------------------------------------------------------------------- family 2
FAR_QUERY_DIST = (0.5, 3.0, 40.0)
FAR_QUERY_DIR = np.array([1.0, -2.0, 0.5]) / np.linalg.norm([1.0, -2.0, 0.5])


@functools.lru_cache(maxsize=None)
def centred_patch():
    """the patch recentred on the origin: maxabs ~ 0.1"""
    p = patch8000().astype(np.float64)
    mid = 0.5 * (p.min(0) + p.max(0))
    return np.ascontiguousarray((p - mid).astype(np.float32))


@functools.lru_cache(maxsize=None)
def far_query_source(dist: float):
    return shifted(centred_patch(), (dist * FAR_QUERY_DIR).astype(np.float32))


# ------------------------------------------------------------------------------- family 3
ROT_ANGLES = (0.5, math.pi / 2, 3.1)


@functools.lru_cache(maxsize=None)
def rotated_pair(angle: float):
    """(source, target = G cad, T = float32(G Ttrue^-1)): G = rotation by `angle` about PART_AXIS through
    the part's centre plus a translation"""
    from leica_point_cloud_processing_amd import synth

    src, cad, Ttrue = part6000()
    G = synth.axis_angle_matrix(PART_AXIS, angle, synth.PART_CENTER, (0.2, -0.1, 0.3))
    tgt = (cad.astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
    T = (G @ np.linalg.inv(Ttrue)).astype(np.float32)
    return src, np.ascontiguousarray(tgt), T


def rotated_states():
    """x of the objective passes: one fixed, five with angles uniform in (-pi, pi), millimetre translations"""
    rng = np.random.default_rng(23)
    xs = [np.array([0.001, -0.002, 0.0005, 2.0, -1.2, 0.7])]
    for _ in range(5):
        xs.append(np.concatenate([rng.normal(0.0, 2e-3, 3), rng.uniform(-math.pi, math.pi, 3)]))
    return xs


# ------------------------------------------------------------------------------- family 4
BOUNDARY_SIZES = (21, 63, 64, 65, 1023, 1024, 1025, 2049)
CHUNK_PTS = 1024  # the engine's kChunkPts: one wave sums one chunk of the grid-sorted source


@functools.lru_cache(maxsize=None)
def part20000():
    from leica_point_cloud_processing_amd import synth

    return synth.scan_vs_cad(20000, 20000)


def boundary_pair(n: int, nt: int = 4999):
    scan, cad, Ttrue = part20000()
    return np.ascontiguousarray(scan[:n]), np.ascontiguousarray(cad[:nt]), Ttrue


@functools.lru_cache(maxsize=None)
def split_source():
    """4096 scan points, those above the median z moved up by 0.5 m: the grid order is z-major, so the
    moved half sorts last and fills whole chunks the gate rejects"""
    scan, cad, Ttrue = part20000()
    s = scan[:4096].copy()
    up = s[:, 2] > np.median(s[:, 2])
    s[up, 2] += np.float32(0.5)
    return np.ascontiguousarray(s), np.ascontiguousarray(cad[:4999]), Ttrue


# ------------------------------------------------------------------------------- family 5
@functools.lru_cache(maxsize=None)
def degenerate_clouds():
    same = np.tile(np.float32([0.3, 0.4, 0.5]), (40, 1))
    t = (np.arange(200, dtype=np.float64) * 0.01)
    line = np.stack([t, np.zeros(200), np.zeros(200)], 1).astype(np.float32)
    diag = np.stack([t, t, t], 1).astype(np.float32) / np.float32(math.sqrt(3.0))
    # apart from one another by far more than any 20-neighbourhood's reach (19 cm along a line)
    mix = np.concatenate([same, shifted(line, (0.0, 1.0, 0.0)), shifted(diag, (0.0, 0.0, 2.0))])
    return {"same": np.ascontiguousarray(same), "line": line, "diag": np.ascontiguousarray(diag),
            "mix": np.ascontiguousarray(mix)}


# ------------------------------------------------------------------------------- family 6
DUMBBELL_GATE = 0.04


@functools.lru_cache(maxsize=None)
def dumbbell():
    """(target, queries, index ranges of the query groups)"""
    rng = np.random.default_rng(17)
    u = np.ones(3) / math.sqrt(3.0)
    c0 = np.array([0.5, 0.5, 0.5])
    c1 = c0 + 2.0 * u
    tgt = np.concatenate([c0 + rng.normal(0, 0.02, (8000, 3)), c1 + rng.normal(0, 0.02, (8000, 3))]).astype(np.float32)
    mid = 0.5 * (c0 + c1)
    d = rng.normal(size=(600, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    ball = mid + d * (0.05 * rng.uniform(0, 1, (600, 1)) ** (1 / 3))
    seg = c0 + rng.uniform(0, 1, (600, 1)) * (c1 - c0) + rng.normal(0, 1e-3, (600, 3))
    inside = np.concatenate([c0 + rng.normal(0, 0.015, (376, 3)), c1 + rng.normal(0, 0.015, (376, 3))])
    # just outside each bbox face (over a dense part of it: beside a blob) and two corners, at 0.5 / 1 / 2
    # gates -- either side of the gate's decision
    lo, hi = tgt.astype(np.float64).min(0), tgt.astype(np.float64).max(0)
    faces = []
    for m in (0.5, 1.0, 2.0):
        g = m * DUMBBELL_GATE
        for ax in range(3):
            for side, c in ((0, c0), (1, c1)):
                q = np.tile(c, (2, 1)) + rng.normal(0, 0.01, (2, 3))
                q[:, ax] = lo[ax] - g if side == 0 else hi[ax] + g
                faces.append(q)
        faces.append(np.array([lo - g, hi + g]))
        faces.append(np.array([[lo[0] - g, hi[1] + g, lo[2] - g], [hi[0] + g, lo[1] - g, hi[2] + g]]))
    faces = np.concatenate(faces)
    q = np.concatenate([ball, seg, inside, faces]).astype(np.float32)
    assert len(q) == 2000, len(q)
    groups = {"ball": (0, 600), "segment": (600, 1200), "inside": (1200, 1952), "faces": (1952, 2000)}
    return np.ascontiguousarray(tgt), np.ascontiguousarray(q), groups


# ------------------------------------------------------------------------ float32 brute force
def d2_rows(q: np.ndarray, pts: np.ndarray, block: int = 256):
    """rows of float32 squared distances in FLANN's L2_Simple order ((dx dx + dy dy) + dz dz, no FMA),
    `block` queries at a time"""
    q = np.asarray(q, np.float32)
    pts = np.asarray(pts, np.float32)
    px, py, pz = (np.ascontiguousarray(pts[:, a])[None, :] for a in range(3))
    for s in range(0, len(q), block):
        b = q[s:s + block]
        d2 = b[:, 0:1] - px
        d2 *= d2
        for a, p in ((1, py), (2, pz)):
            d = b[:, a:a + 1] - p
            d *= d
            d2 += d
        yield s, d2


def resolution_bruteforce(xyz: np.ndarray) -> float:
    """Utils::computeCloudResolution: mean of the float32 sqrt of the second smallest float32 d2 (the
    smallest is the point itself; an exact duplicate gives 0)"""
    second = np.empty(len(xyz), np.float32)
    for s, d2 in d2_rows(xyz, xyz):
        second[s:s + len(d2)] = np.partition(d2, 1, axis=1)[:, 1]
    return float(np.sqrt(second).astype(np.float64).mean())


def radius_keep_bruteforce(xyz: np.ndarray, radius: float, min_neighbors: int = 3) -> np.ndarray:
    """>= min_neighbors points (self included) with float32 d2 < float32(radius^2)"""
    r2 = np.float32(radius * radius)
    keep = np.zeros(len(xyz), bool)
    for s, d2 in d2_rows(xyz, xyz):
        keep[s:s + len(d2)] = (d2 < r2).sum(axis=1) >= min_neighbors
    return keep


def nearest_d2_bruteforce(q: np.ndarray, pts: np.ndarray) -> np.ndarray:
    out = np.empty(len(q), np.float32)
    for s, d2 in d2_rows(q, pts):
        out[s:s + len(d2)] = d2.min(axis=1)
    return out


def duplicates_and_ties(xyz: np.ndarray, k: int = 20):
    """(points with an exact duplicate, points whose k-NN set -- the point itself included, as PCL's
    computeCovariances asks for it -- is decided by a tie: equal float32 d2 at ranks k and k + 1)"""
    dup = tie = 0
    for s, d2 in d2_rows(xyz, xyz):
        part = np.sort(np.partition(d2, k, axis=1)[:, :k + 1], axis=1)
        dup += int((part[:, 1] == 0).sum())
        tie += int((part[:, k - 1] == part[:, k]).sum())
    return dup, tie


def oracle(src, tgt, **kw):
    from oracle import ref

    o = ref.RefGICP(**kw)
    o.set_source(src)
    o.set_target(tgt)
    return o

"""The map stacks of the information-gain tests (tests/test_gpu_infogain.py compares the kernels with the definition on them,
tests/test_infogain_host.py checks that they reach what they are for) and their references, computed once.  The frontier tests'
stacks (tests/frontier_cases.py) are reused where they fit; the new ones have walls, so that rays stop."""
import functools

import numpy as np

import frontier_cases as fc
from nextbestpath_amd.utility import infogain as ig


def blocks_item(S, seed, band):
    """Seen space as a chequerboard of 16-pixel blocks hit at 60 % (the closing fills them and leaves the other blocks unknown), the
    band on `band` of all pixels, seen or not; content in row 0 and column 0, which changes nothing."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    seen = (((r // 16) + (c // 16)) % 2 == 0) & (rng.random((S, S)) < 0.6)
    m = np.zeros((6, S, S), np.float32)
    ch = rng.integers(0, 5, (S, S))
    for k in range(5):
        m[k][seen & (ch == k)] = 1.0 + k
    m[5][rng.random((S, S)) < band] = 2.0
    m[:, 0, :] = rng.integers(0, 2, (6, S))
    m[:, :, 0] = rng.integers(0, 2, (6, S))
    return m


def room(door, S=64):
    """Seen free space inside a 17-pixel ring of band pixels around rows and columns 24..40, unknown outside; `door`: the pixel
    (24, 32) of the north wall is taken out (and stays unseen)."""
    m = np.zeros((6, S, S), np.float32)
    m[0, 25:40, 25:40] = 1.0
    m[5, 24, 24:41] = m[5, 40, 24:41] = m[5, 24:41, 24] = m[5, 24:41, 40] = 1.0
    if door:
        m[5, 24, 32] = 0.0
    return m


def stairs(gap, S=64):
    """The staircase wall r + c == 70 (8-connected only) with seen free space on r + c < 70 and unknown space beyond; `gap`: the wall
    pixel (35, 35) is taken out (and stays unseen)."""
    r, c = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    m = np.zeros((6, S, S), np.float32)
    m[0][r + c < 70] = 1.0
    m[5][r + c == 70] = 1.0
    if gap:
        m[5, 35, 35] = 0.0
    return m


def _seam_case():
    """S = 128 (two words per row), B = 3.  Item 0: a seen free corridor along rows 60..68 through all columns, so across the seam
    between columns 63 and 64, walled in by band rows with door gaps, in unknown space; vertical walls at columns 63 and 64, a diagonal wall across the seam.
    Item 1: the frontier tests' seam item with its band block across the seam.  Item 2: blocks with a sparse band."""
    S = 128
    m = np.zeros((3, 6, S, S), np.float32)
    m[0, 1, 60:69, 1:] = 1.0
    m[0, 2, 1:, 60:69] = 1.0
    m[0, 5, 59, 1:] = m[0, 5, 69, 1:] = 1.0
    m[0, 5, 1:, 59] = m[0, 5, 1:, 69] = 1.0
    m[0, 5, 60:69, 60:69] = 0.0                            # the crossing is open
    for k in (5, 30, 62, 63, 64, 65, 100, 126):            # door gaps, some of them at the seam
        m[0, 5, 59, k] = m[0, 5, 69, k] = m[0, 5, k, 59] = m[0, 5, k, 69] = 0.0
    m[0, 5, 20:40, 63] = 1.0                               # walls on either side of the seam, far from the corridor
    m[0, 5, 90:110, 64] = 1.0
    for i in range(24):                                    # a diagonal wall (8-connected only) across the seam
        m[0, 5, 74 + i, 52 + i] = 1.0
    m[1] = fc.case("seam")[1]
    m[2] = blocks_item(S, 7, 0.005)
    return m


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "one_word":
        return np.stack([blocks_item(64, 1, 0.03)])
    if name == "seam":
        return _seam_case()
    if name == "s256":
        return np.stack([blocks_item(256, 2, 0.005), blocks_item(256, 3, 0.03)])
    if name == "bands":                                    # band density 0, 0.5 %, 3 %, 15 % and full
        items = [blocks_item(128, 20 + i, p) for i, p in enumerate((0.0, 0.005, 0.03, 0.15, 1.0))]
        return np.stack(items)
    if name == "frontier_dense":                           # the frontier tests' 15 % band on random seen pixels
        return fc.case("density50")
    if name == "empty":
        return fc.case("empty")
    if name == "rooms":
        return np.stack([room(False), room(True), stairs(False), stairs(True)])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, R, d, unknown, penalty):
    return ig.policy_batch(case(name), radius=R, dilate=d, unknown=unknown, distance_penalty=penalty)


def edge_cells(B, V):
    """(b, g0, g1): the centre, the four edges and the four corners of the last map, the cells beside them, one cell of every map."""
    h, e = V // 2, V - 1
    cells = [(B - 1, g0, g1) for g0 in (0, 1, h, e) for g1 in (0, 1, h - 1, e)]
    cells += [(b, h, h) for b in range(B)] + [(0, 5, 15), (0, e, 3)]
    return np.asarray(cells, np.int32)


def corner_cuts(blocked, R, g0, g1):
    """How many rays of cell (g0, g1) the corner rule stops (a diagonal step to an open pixel between two blocked corners)."""
    S = blocked.shape[0]
    at = lambda r, c: not (0 <= r < S and 0 <= c < S) or bool(blocked[r, c])
    r0, c0 = 4 * g0, 4 * g1
    if at(r0, c0):
        return 0
    n = 0
    for ray in ig.ray_table(R):
        qr, qc = r0, c0
        for dy, dx in ray:
            pr, pc = r0 + int(dy), c0 + int(dx)
            if at(pr, pc):
                break
            if pr != qr and pc != qc and at(pr, qc) and at(qr, pc):
                n += 1
                break
            qr, qc = pr, pc
    return n


# (case, R, d, unknown, penalty): R in {1, 2, 24, 31} and d in {0, 2, 8} on every kind of case, both modes, both penalties
POLICY_CASES = [
    ("one_word", 1, 0, "free", 0), ("one_word", 2, 2, "obstacle", 3), ("one_word", 24, 8, "obstacle", 0), ("one_word", 31, 0, "free", 3),
    ("seam", 1, 2, "obstacle", 0), ("seam", 2, 0, "free", 3), ("seam", 24, 2, "free", 0), ("seam", 31, 0, "obstacle", 3),
    ("seam", 31, 8, "obstacle", 0),
    ("s256", 31, 2, "obstacle", 1),
    ("bands", 1, 0, "obstacle", 0), ("bands", 2, 8, "free", 3), ("bands", 24, 2, "obstacle", 0), ("bands", 31, 0, "obstacle", 3),
    ("frontier_dense", 24, 0, "free", 0), ("frontier_dense", 31, 2, "obstacle", 3),
    ("empty", 31, 0, "obstacle", 0), ("empty", 2, 8, "free", 3),
    ("rooms", 31, 0, "obstacle", 0), ("rooms", 24, 2, "free", 3), ("rooms", 2, 0, "free", 0), ("rooms", 1, 8, "obstacle", 0),
]

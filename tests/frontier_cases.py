"""The map stacks of the frontier tests (tests/test_gpu_frontier.py compares the kernels with the definition on them,
tests/test_frontier_host.py checks that they reach what they are for) and their references, computed once."""
import functools

import numpy as np

from nextbestpath_amd.utility import frontier as fr


def random_item(S, seed, density):
    rng = np.random.default_rng(seed)
    m = np.zeros((6, S, S), np.float32)
    seen = rng.random((S, S)) < density
    ch = rng.integers(0, 5, (S, S))
    for k in range(5):
        m[k][seen & (ch == k)] = 1.0 + k
    m[5][rng.random((S, S)) < 0.15] = 2.0              # the band, on seen and unseen pixels alike
    m[:, 0, :] = rng.integers(0, 2, (6, S))            # content outside the domain: changes nothing
    m[:, :, 0] = rng.integers(0, 2, (6, S))
    return m


def _seam_case():
    """S = 128 (two words per row), B = 3: runs that end at columns 63, 64, 65 and 127, and frontier pixels in rows and columns
    1 and S - 1."""
    S = 128
    m = np.zeros((3, 6, S, S), np.float32)
    ends = (63, 64, 65, 127)
    for i, e in enumerate(ends):                       # item 0: seen runs (3 rows thick) in unseen space
        m[0, i % 5, 10 + 12 * i:13 + 12 * i, 40:e + 1] = 1.0
        m[0, 1, 70 + 12 * i, e - 2:e + 1] = 1.0        # ... and thin ones
    m[1, 0, 1:, 1:] = 1.0                              # item 1: unseen runs in seen space
    for i, e in enumerate(ends):
        m[1, :, 10 + 12 * i:13 + 12 * i, 40:e + 1] = 0
        m[1, :, 70 + 12 * i, e - 2:e + 1] = 0
    m[1, 5, 40:60, 60:70] = 1.0                        # a band block across the seam
    for r0 in (1, S - 3):                              # item 2: free blocks in the four corners and along the four edges
        for c0 in (1, 62, S - 3):
            m[2, 3, r0:r0 + 3, c0:c0 + 3] = 1.0
            m[2, 3, c0:c0 + 3, r0:r0 + 3] = 1.0
    f = fr.cell_classes(m[2], 0)["frontier"]
    assert f[1].any() and f[S - 1].any() and f[:, 1].any() and f[:, S - 1].any()
    return m


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "one_word":
        return np.stack([random_item(64, 1, 0.3)])
    if name == "seam":
        return _seam_case()
    if name == "s256":
        return np.stack([random_item(256, 2, 0.02), random_item(256, 3, 0.6)])
    if name == "empty":
        return np.zeros((2, 6, 64, 64), np.float32)
    if name == "full":
        m = np.ones((2, 6, 128, 128), np.float32)
        m[:, 5] = 0
        m[1, 5, 30:40, 60:70] = 1.0
        return m
    if name.startswith("density"):
        p = {"density01": 0.01, "density50": 0.5, "density99": 0.99}[name]
        return np.stack([random_item(128, 10 + i, p) for i in range(3)])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def classes(name, d):
    cls = [fr.cell_classes(m, d) for m in case(name)]
    return np.stack([c["frontier"] for c in cls]), np.stack([c["unknown"] for c in cls])


@functools.lru_cache(maxsize=None)
def reference(name, R, d, unknown, penalty):
    return fr.policy_batch(case(name), radius=R, dilate=d, unknown=unknown, distance_penalty=penalty)


# (case, R, d, unknown, penalty): every case at the window's and the dilation's extremes, both modes, both penalties
POLICY_CASES = [
    ("one_word", 1, 0, "free", 0), ("one_word", 2, 1, "obstacle", 3), ("one_word", 31, 8, "obstacle", 0), ("one_word", 24, 2, "free", 3),
    ("seam", 1, 0, "obstacle", 0), ("seam", 2, 1, "free", 3), ("seam", 31, 0, "obstacle", 3), ("seam", 31, 8, "obstacle", 0),
    ("seam", 24, 2, "free", 0),
    ("s256", 31, 1, "obstacle", 0), ("s256", 2, 8, "free", 3), ("s256", 1, 0, "obstacle", 3), ("s256", 24, 2, "obstacle", 0),
    ("empty", 31, 0, "obstacle", 0), ("empty", 2, 8, "free", 3), ("full", 31, 8, "obstacle", 3), ("full", 1, 0, "free", 0),
    ("density01", 31, 0, "obstacle", 0), ("density01", 2, 8, "obstacle", 3), ("density01", 24, 1, "free", 0),
    ("density50", 31, 1, "obstacle", 3), ("density50", 1, 0, "free", 0), ("density50", 24, 8, "obstacle", 0),
    ("density99", 31, 0, "obstacle", 0), ("density99", 2, 1, "free", 3), ("density99", 31, 8, "obstacle", 3),
]

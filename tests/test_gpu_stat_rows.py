"""GPU: the ORDER of the fixed-order statistics fold (csrc/nbp_stat_rows.h under hipops.recon_stats / view_stats / tsdf_stats).

The other tests of these summaries allow 1e-10 on the float64 sums and ask two runs to agree: any fixed order passes them.  Here
the order itself is restated in numpy and the float64 sums must equal it BIT FOR BIT (the counts exactly):

  * thread t of block b adds its elements b 256 + t, b 256 + t + B 256, ... in index order (B blocks of 256 threads);
  * inside a wave of 64 the tree `a[:off] += a[off:2 off]` for off = 32, 16, ..., 1 (what lane 0 of a __shfl_down tree holds);
  * the four waves of a block in order, ((w0 + w1) + w2) + w3: one row per block;
  * the B rows in index order, from 0.0.

B = 256 for recon and TSDF, 32 per view for the view statistics.  The element counts straddle every seam of that geometry: one
element, either side of a wave (64), of a block (256) and of the whole launch (B 256).  No elements at all exist for recon only (an
image has H, W >= 2, a volume at least one voxel).  The inputs span several orders of magnitude, so that another order gives other
bits: the test asserts that numpy's own (pairwise) sum differs on the largest case, which keeps it able to fail.  The TSDF
statistics are integer counts: no order to pin, only the seams."""
import numpy as np
import pytest
import torch

from nextbestpath_amd.utility import recon_metrics as rm
from nextbestpath_amd.utility import tsdf
from nextbestpath_amd.utility import view_metrics as vm

f32 = np.float32
THREADS, WAVE = 256, 64
RECON_BLOCKS, VIEW_BLOCKS, TSDF_BLOCKS = 256, 32, 256


def fold(terms, blocks):
    """The device's sum of `terms` (float64 or int64 [n]) over `blocks` blocks of 256 threads, in its order."""
    terms = np.asarray(terms)
    stride = blocks * THREADS
    rounds = max(1, -(-terms.shape[0] // stride))
    padded = np.zeros(rounds * stride, terms.dtype)              # (x + 0 = x for the non-negative terms of these sums)
    padded[:terms.shape[0]] = terms
    acc = np.zeros(stride, terms.dtype)
    for r in range(rounds):                                      # a thread's strided elements, in index order
        acc = acc + padded[r * stride:(r + 1) * stride]
    a = acc.reshape(blocks, THREADS // WAVE, WAVE).copy()
    off = WAVE // 2
    while off >= 1:                                              # the tree inside a wave
        a[..., :off] += a[..., off:2 * off]
        off //= 2
    waves = a[..., 0]
    rows = waves[:, 0]
    for w in range(1, THREADS // WAVE):                          # the waves in order
        rows = rows + waves[:, w]
    total = terms.dtype.type(0)
    for b in range(blocks):                                      # the rows in order
        total = total + rows[b]
    return total


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _magnitudes(rng, n, lo, hi):
    """n positive float32 values, log-uniform over [10^lo, 10^hi]."""
    return (10.0 ** rng.uniform(lo, hi, n)).astype(f32)


# ---- recon
RECON_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, RECON_BLOCKS * THREADS - 1, RECON_BLOCKS * THREADS, RECON_BLOCKS * THREADS + 1]
RECON_THRESHOLDS = (0.01, 1.0, 30.0)


@pytest.fixture(scope="module")
def recon_values():
    return _magnitudes(np.random.default_rng(71), max(RECON_SIZES), -6, 4)


def _recon_want(v):
    d = v.astype(np.float64)
    sums = np.array([fold(np.sqrt(d), RECON_BLOCKS), fold(d, RECON_BLOCKS)], np.float64)
    counts = [int(fold((v <= rm.sq_below(t)).astype(np.int64), RECON_BLOCKS)) for t in RECON_THRESHOLDS]
    return sums, counts


def test_recon_inputs_make_the_order_matter(recon_values):
    d = recon_values.astype(np.float64)
    sums, counts = _recon_want(recon_values)
    assert _bits(np.sqrt(d).sum()) != _bits(sums[0]) and _bits(d.sum()) != _bits(sums[1])
    assert counts == rm.stats_reference(recon_values, RECON_THRESHOLDS)[1].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("n", RECON_SIZES)
def test_recon_stats_fold_order_bit_for_bit(hip, recon_values, n):
    from nextbestpath_amd.utility import hipops
    v = recon_values[:n]
    want_sums, want_counts = _recon_want(v)
    sums, counts = hipops.recon_stats(_dev(v), RECON_THRESHOLDS)
    sums = sums.cpu().numpy()
    print(n, sums, want_sums, counts.tolist(), want_counts)
    assert counts.tolist() == want_counts
    assert np.array_equal(_bits(sums), _bits(want_sums))


# ---- views: (H, W) with H W on either side of 64, 256 and 32 x 256 per view
VIEW_SHAPES = [(2, 2), (3, 21), (2, 32), (5, 13), (3, 85), (16, 16), (2, 129), (2, 4095), (64, 128), (3, 2731)]
VIEW_V, VIEW_TAU, VIEW_CLOUD = 3, 50.0, 1000


def _view_case(H, W):
    """Keys, depth and colour images made directly (no splat): most pixels hit, with depths over three orders of magnitude and |dz| over
    five (more would leave the sum to its few largest terms, and two orders would often round alike); some empty,
    some without ground truth, some off by more than the tolerance either way."""
    rng = np.random.default_rng(1000 * H + W)
    n = VIEW_V * H * W
    z_c = _magnitudes(rng, n, -1, 2)
    kind = rng.integers(0, 16, n)
    z_c[kind >= 12] *= f32(1e-7)                                     # (without these sum |dz| is exact in float64, in any order)
    dz = (z_c * _magnitudes(rng, n, -3, -0.3) * rng.choice(np.array([-1, 1], f32), n)).astype(f32)
    z_gt = (z_c - dz).astype(f32)
    z_c[kind == 0], z_gt[kind == 0] = f32(500), f32(100)             # a leak
    z_c[kind == 1], z_gt[kind == 1] = f32(100), f32(500)             # a floater
    z_gt[kind == 2] = f32(-1)
    index = rng.integers(0, VIEW_CLOUD, n).astype(np.uint64)
    keys = (z_c.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index
    keys[kind == 3] = vm.EMPTY
    shape = (VIEW_V, H, W)
    cloud_rgb = _magnitudes(rng, 3 * VIEW_CLOUD, -3, 0).reshape(VIEW_CLOUD, 3)
    rgb_gt = rng.uniform(0, 1, shape + (3,)).astype(f32)
    return keys.reshape(shape), z_gt.reshape(shape), cloud_rgb, rgb_gt


def _view_want(keys, z_gt, cloud_rgb, rgb_gt):
    z_c, index, rgb_c = vm.resolve(keys, cloud_rgb)
    cl = vm.classify(z_c, z_gt, VIEW_TAU, np.inf)
    V = keys.shape[0]
    counts = np.zeros((V, 6), np.int64)
    sums = np.zeros((V, 3), np.float64)
    for v in range(V):
        for k, name in enumerate(("gt", "c", "hit", "hole", "leak", "floater")):
            counts[v, k] = fold(cl[name][v].reshape(-1).astype(np.int64), VIEW_BLOCKS)
        hit = cl["hit"][v].reshape(-1)
        d = z_c[v].reshape(-1).astype(np.float64) - z_gt[v].reshape(-1).astype(np.float64)
        e = rgb_c[v].reshape(-1, 3).astype(np.float64) - rgb_gt[v].reshape(-1, 3).astype(np.float64)
        e2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        for k, term in enumerate((np.abs(d), d * d, e2)):
            sums[v, k] = fold(np.where(hit, term, 0.0), VIEW_BLOCKS)
    return counts, sums


def test_view_inputs_make_the_order_matter():
    keys, z_gt, cloud_rgb, rgb_gt = _view_case(*VIEW_SHAPES[-1])
    counts, sums = _view_want(keys, z_gt, cloud_rgb, rgb_gt)
    z_c, _, rgb_c = vm.resolve(keys, cloud_rgb)
    ref_counts, ref_sums = vm.raw_stats(z_c, rgb_c, z_gt, rgb_gt, VIEW_TAU, np.inf)
    assert np.array_equal(counts, ref_counts) and np.all(counts[:, 2] > 0.5 * keys[0].size)
    differs = _bits(ref_sums) != _bits(sums)                         # (two orders may round alike on one sum: 8 of these 9 do not)
    assert np.all(differs.any(0)) and differs.sum() >= 6
    assert np.all(np.abs(ref_sums - sums) <= 1e-10 * sums)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", VIEW_SHAPES)
def test_view_stats_fold_order_bit_for_bit(hip, H, W):
    from nextbestpath_amd.utility import hipops
    keys, z_gt, cloud_rgb, rgb_gt = _view_case(H, W)
    want_counts, want_sums = _view_want(keys, z_gt, cloud_rgb, rgb_gt)
    counts, sums = hipops.view_stats(_dev(keys.view(np.int64)), _dev(cloud_rgb), _dev(z_gt), _dev(rgb_gt), VIEW_TAU)
    counts, sums = counts.cpu().numpy(), sums.cpu().numpy()
    print(H, W, sums, want_sums, counts.tolist())
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(_bits(sums), _bits(want_sums))


# ---- TSDF: volumes of n voxels
TSDF_SIZES = [1, 63, 64, 65, 255, 256, 257, TSDF_BLOCKS * THREADS - 1, TSDF_BLOCKS * THREADS, TSDF_BLOCKS * THREADS + 1]
TSDF_DIMS = {65535: (3, 5, 4369), 65536: (16, 16, 256), 65537: (1, 1, 65537)}


@pytest.mark.gpu
@pytest.mark.parametrize("n", TSDF_SIZES)
def test_tsdf_stats_counts_at_the_seams(hip, n):
    from nextbestpath_amd.utility import hipops
    rng = np.random.default_rng(n)
    dims = TSDF_DIMS.get(n, (1, 1, n))
    assert dims[0] * dims[1] * dims[2] == n
    vol = np.zeros(dims + (2,), np.int32)
    vol[..., 1] = rng.integers(0, 4, dims)
    vol[..., 0] = rng.integers(-130, 131, dims) * vol[..., 1]        # |S| around 127 W: both sides of the usable rule
    min_weight = 2
    observed = vol[..., 1].reshape(-1) > 0
    usable = tsdf.usable_mask(vol, min_weight).reshape(-1)
    want = [int(fold(observed.astype(np.int64), TSDF_BLOCKS)), int(fold(usable.astype(np.int64), TSDF_BLOCKS))]
    ref = tsdf.stats(vol, min_weight)
    assert want == [ref["observed_voxels"], ref["usable_voxels"]]
    got = hipops.tsdf_stats(_dev(vol), min_weight).tolist()
    print(n, got, want)
    assert got == want

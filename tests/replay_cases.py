"""Shared inputs of the compact-replay tests (test_replay_codec_host.py, test_gpu_replay_codec.py): planes that sit on every edge of
the width selection of nextbestpath_amd/utility/replay_codec.py, and records built from them."""
import numpy as np


def channel_cases(S, seed=0):
    """[(name, plane [S,S] fp32, width)]: one plane per case of the format's width table."""
    rng = np.random.default_rng(1000 * S + seed)
    SS = S * S

    def sparse(values, density=0.07):
        """zeros with counts 1..9 sprinkled in, then `values` at distinct random places"""
        p = np.where(rng.random(SS) < density, rng.integers(1, 10, SS), 0).astype(np.float32)
        at = rng.choice(SS, len(values), replace=False)
        p[at] = np.asarray(values, np.float32)
        return p.reshape(S, S)

    only_neg_zero = np.zeros(SS, np.float32)
    only_neg_zero[rng.choice(SS, 5, replace=False)] = -0.0
    cases = [
        ("all_zero", np.zeros((S, S), np.float32), 0),
        ("all_nonzero", rng.integers(1, 201, (S, S)).astype(np.float32), 1),
        ("all_ones", np.ones((S, S), np.float32), 0),
        ("sparse_ones", (rng.random((S, S)) < 0.1).astype(np.float32), 0),
        ("has_255", sparse([255.0]), 1),
        ("has_256", sparse([256.0]), 2),
        ("has_65535", sparse([65535.0, 255.0]), 2),
        ("has_65536", sparse([65536.0]), 4),
        ("non_integer", sparse([2.5]), 4),
        ("negative", sparse([-3.0]), 4),
        ("neg_zero", only_neg_zero.reshape(S, S), 4),
        ("nan", sparse([np.nan]), 4),
        ("denormal", sparse([np.float32(1e-42)]), 4),
        ("first_and_last", sparse([], 0.0), 0),
    ]
    cases[-1][1].flat[[0, SS - 1]] = 1.0
    return cases


def case_records(S, seed=0):
    """-> (rec [m,6,S,S] fp32, widths [m][6]): every channel case once, six to a record (the last one padded with zero planes),
    then one record with a different width in every neighbouring channel (0, 1, 2, 4, 2, 0)."""
    cases = channel_cases(S, seed)
    planes = [p for _, p, _ in cases]
    widths = [w for _, _, w in cases]
    while len(planes) % 6:
        planes.append(np.zeros((S, S), np.float32))
        widths.append(0)
    by = {name: p for name, p, _ in cases}
    planes += [by["sparse_ones"], by["has_255"], by["has_256"], by["non_integer"], by["has_65535"], by["all_ones"]]
    widths += [0, 1, 2, 4, 2, 0]
    rec = np.stack(planes).reshape(-1, 6, S, S)
    return rec, np.asarray(widths).reshape(-1, 6).tolist()


def records(S, n, seed=0):
    """n records [n,6,S,S]: the case records, over and over with fresh random places."""
    out, k = [], 0
    while len(out) < n:
        out.extend(case_records(S, seed + k)[0])
        k += 1
    return np.ascontiguousarray(np.stack(out[:n]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)

"""Training data path -- host-side mirror of next_best_path/utility/nbp_utils.py: the replay store
(store_experience :32-44, store_validation_data :78-100, read_random_data_readonly :63-76, read_combined_data
:103-141) and the exploration-with-hindsight trajectory collection that fills it (trajectory_collection :470-852).

Record schema and value encoding are the reference's: a msgpack map with 'current_model_input' [1,5,S,S] f32,
'current_gt_2d_layout' [1,1,S,S] f32, 'target_value_map_pixel' [K,3] i64 (heading, row, col),
'actual_coverage_gain' [K] f32, 'pose_i'; arrays in msgpack-numpy's {nd, type, kind, shape, data} form; keys are
zero-padded millisecond timestamps (`%012d`, 13 digits today).  The container is LMDB: through the `lmdb` module when it is importable,
otherwise through this package's own reader / writer of LMDB's file format (MdbEnv -> csrc/nbp_mdb.cpp; lmdb is not installable in this
image; msgpack-numpy is absent too, hence the explicit encoder below).  LogEnv (an append-only log, rounds 2-5) still opens its own files.

All map work of the collection (cloud accumulation, slab maps, trajectory image, GT obstacle label, coverage,
rendering, un-projection, NBP forward) runs on the HIP kernels; the host keeps the reference's control flow:
Boltzmann goal sampling, uniform-cost search on the mesh-free lattice edges, 60 % random headings, hindsight
relabelling of every (earlier, later) pair of a finished path.
"""
from __future__ import annotations

import math
import os
import random
import struct
import time

import msgpack
import numpy as np
import torch

from ..simulator import lockstep
from ..simulator import scene as sim_scene
from . import hipops
from . import planner_host
from . import replay_codec
from . import utils as hu
from .long_term_utils import LatticePlanner


# ------------------------------------------------------------------ record encoding (msgpack-numpy layout)
def _encode(obj):
    if isinstance(obj, np.ndarray):
        return {b"nd": True, b"type": obj.dtype.str, b"kind": b"", b"shape": list(obj.shape),
                b"data": np.ascontiguousarray(obj).tobytes()}
    if isinstance(obj, (np.bool_, np.number)):
        return {b"nd": False, b"type": obj.dtype.str, b"data": obj.tobytes()}
    raise TypeError(f"cannot pack {type(obj)}")


def _decode(obj):
    nd = obj.get(b"nd", obj.get("nd"))
    if nd is None:
        return obj
    g = lambda k: obj.get(k.encode(), obj.get(k))
    dt = g("type")
    dt = np.dtype(dt.decode() if isinstance(dt, bytes) else dt)
    if nd:
        return np.frombuffer(g("data"), dtype=dt).reshape(g("shape")).copy()
    return np.frombuffer(g("data"), dtype=dt)[0]


REPLAY_FORMATS = ("reference", "compact")


def check_replay_format(replay_format):
    if replay_format not in REPLAY_FORMATS:
        raise ValueError(f"replay_format {replay_format!r}: expected one of {REPLAY_FORMATS}")
    return replay_format


def _stream_of(data) -> bytes:
    """The compact stream a record dict carries under 'nbpc' (bytes, or a uint8 array / host tensor that starts with it)."""
    st = data["nbpc"]
    if isinstance(st, (bytes, bytearray)):
        return bytes(st)
    a = st.detach().cpu().numpy() if isinstance(st, torch.Tensor) else np.asarray(st)
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    return a[:replay_codec.used_bytes(a)].tobytes()


def pack_record(data, replay_format="reference") -> bytes:
    """ref :35-41 (tensors -> numpy -> msgpack with use_bin_type).  replay_format "reference" (the default): the reference's
    bytes.  "compact": the same map with the two image arrays replaced by key 'nbpc', the record's compact stream
    (utility/replay_codec.py; lossless) -- the one `data` carries under 'nbpc', else the numpy codec's from its arrays."""
    check_replay_format(replay_format)
    np_ = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    small = {
        "target_value_map_pixel": np_(data["target_value_map_pixel"]),
        "actual_coverage_gain": np_(data["actual_coverage_gain"]),
        "pose_i": np.array(data["pose_i"]),
    }
    if replay_format == "compact":
        stream = _stream_of(data) if "nbpc" in data else replay_codec.encode(np_(data["current_model_input"]),
                                                                             np_(data["current_gt_2d_layout"]))
        return msgpack.packb({"nbpc": stream, **small}, use_bin_type=True, default=_encode)
    if "nbpc" in data and "current_model_input" not in data:
        x, gt = replay_codec.decode(_stream_of(data))
    else:
        x, gt = np_(data["current_model_input"]), np_(data["current_gt_2d_layout"])
    return msgpack.packb({"current_model_input": x, "current_gt_2d_layout": gt, **small}, use_bin_type=True, default=_encode)


def unpack_record(value: bytes, keep_compact=False):
    """A stored value -> the record dict.  The record itself says how it is read: a reference-format one comes back as ever,
    whatever the flag; a compact one comes back with the same five keys, its images decoded by the numpy codec -- or, with
    keep_compact, as {'nbpc': stream, 'S': side, + the three small keys} after the stream's header has been validated (the
    trainer expands such records on the device, hipops.replay_decode)."""
    rec = msgpack.unpackb(value, object_hook=_decode, raw=False, strict_map_key=False)
    rec["pose_i"] = int(np.asarray(rec["pose_i"]))
    if "nbpc" in rec:
        if keep_compact:
            rec["S"] = replay_codec.parse_header(rec["nbpc"])[0]
            return rec
        stream = rec.pop("nbpc")
        x, gt = replay_codec.decode(stream)
        rec = {"current_model_input": x, "current_gt_2d_layout": gt, **rec}
    return rec


def expand_record(rec):
    """A record as unpack_record(..., keep_compact=True) returns it -> the five-key form (host decode); others pass through."""
    if "nbpc" not in rec:
        return rec
    rest = {k: v for k, v in rec.items() if k not in ("nbpc", "S")}
    x, gt = replay_codec.decode(rec["nbpc"])
    return {"current_model_input": x, "current_gt_2d_layout": gt, **rest}


# ------------------------------------------------------------------ containers
class LogEnv:
    """Append-only key/value log with LMDB's ordered-cursor semantics for the few calls the trainer makes.
    File layout: repeated [u16 key length][key][u32 length][payload]; length 0xFFFFFFFF marks a deleted key."""

    def __init__(self, path):
        os.makedirs(path, exist_ok=True)
        self.file = os.path.join(path, "data.log")
        self.index = {}          # key -> (offset, length)
        if os.path.exists(self.file):
            with open(self.file, "rb") as fh:
                while True:
                    kl = fh.read(2)
                    if len(kl) < 2:
                        break
                    klen = struct.unpack("<H", kl)[0]
                    head = fh.read(klen + 4)
                    if len(head) < klen + 4:
                        break
                    key, n = head[:klen], struct.unpack("<I", head[klen:])[0]
                    if n == 0xFFFFFFFF:
                        self.index.pop(key, None)
                        continue
                    self.index[key] = (fh.tell(), n)
                    fh.seek(n, 1)

    def put(self, key: bytes, value: bytes):
        with open(self.file, "ab") as fh:
            fh.write(struct.pack("<H", len(key)) + key + struct.pack("<I", len(value)))
            off = fh.tell()
            fh.write(value)
        self.index[key] = (off, len(value))

    def delete(self, key: bytes):
        if key in self.index:
            with open(self.file, "ab") as fh:
                fh.write(struct.pack("<H", len(key)) + key + struct.pack("<I", 0xFFFFFFFF))
            del self.index[key]

    def entries(self):
        return len(self.index)

    def keys(self):
        return sorted(self.index)

    def items(self):
        with open(self.file, "rb") as fh:
            for k in self.keys():
                off, n = self.index[k]
                fh.seek(off)
                yield k, fh.read(n)

    def close(self):
        pass


class LmdbEnv:
    """The reference's container (train_nbp_model.py:61-63); used when `lmdb` is importable."""

    def __init__(self, path, map_size):
        import lmdb
        os.makedirs(path, exist_ok=True)
        self.env = lmdb.open(path, map_size=map_size)

    def put(self, key, value):
        with self.env.begin(write=True) as txn:
            txn.put(key, value)

    def delete(self, key):
        with self.env.begin(write=True) as txn:
            txn.delete(key)

    def entries(self):
        return self.env.stat()["entries"]

    def keys(self):
        with self.env.begin(write=False) as txn:
            return [bytes(k) for k, _ in txn.cursor()]

    def items(self):
        with self.env.begin(write=False) as txn:
            for k, v in txn.cursor():
                yield bytes(k), bytes(v)

    def close(self):
        self.env.close()


class MdbEnv:
    """<path>/data.mdb in LMDB's on-disk format through the native container of this package (csrc/nbp_mdb.cpp: nbp_mdb_*), for
    hosts without the `lmdb` module: a store written here opens with lmdb.open(path) and one the reference wrote opens here.  Same
    interface as LmdbEnv / LogEnv; every put / delete is its own committed transaction, as in the reference."""

    def __init__(self, path, map_size=200 * 1024 ** 3, sync=False):
        import ctypes as C
        from .. import _lib
        self._L, self._C = _lib.lib(), C
        os.makedirs(path, exist_ok=True)          # (lmdb.open creates the last component only; the trainers hand over nested paths)
        h = C.c_void_p()
        _lib.check(self._L.nbp_mdb_open(os.fsencode(path), int(map_size), int(bool(sync)), C.byref(h)), "nbp_mdb_open")
        self._h = h

    def put(self, key: bytes, value: bytes):
        rc = self._L.nbp_mdb_put(self._h, key, len(key), value, len(value))
        if rc:
            raise RuntimeError(f"nbp_mdb_put failed ({rc})")

    def delete(self, key: bytes):
        rc = self._L.nbp_mdb_del(self._h, key, len(key))
        if rc not in (0, 1):
            raise RuntimeError(f"nbp_mdb_del failed ({rc})")
        return rc == 0

    def get(self, key: bytes):
        C = self._C
        n = C.c_size_t()
        rc = self._L.nbp_mdb_get(self._h, key, len(key), None, 0, C.byref(n))
        if rc == 1:
            return None
        buf = C.create_string_buffer(max(n.value, 1))
        rc = self._L.nbp_mdb_get(self._h, key, len(key), buf, n.value, C.byref(n))
        if rc:
            raise RuntimeError(f"nbp_mdb_get failed ({rc})")
        return buf.raw[:n.value]

    def entries(self):
        return int(self._L.nbp_mdb_entries(self._h))

    def stat(self):
        out = (self._C.c_ulonglong * 8)()
        self._L.nbp_mdb_stat(self._h, out)
        names = ("depth", "branch_pages", "leaf_pages", "overflow_pages", "entries", "last_pgno", "last_txnid", "psize")
        return dict(zip(names, (int(v) for v in out)))

    def keys(self):
        C = self._C
        n = C.c_size_t()
        self._L.nbp_mdb_keys(self._h, None, 0, C.byref(n))
        buf = C.create_string_buffer(max(n.value, 1))
        self._L.nbp_mdb_keys(self._h, buf, n.value, C.byref(n))
        raw, out, i = buf.raw[:n.value], [], 0
        while i < len(raw):
            k = struct.unpack_from("<H", raw, i)[0]
            out.append(raw[i + 2:i + 2 + k])
            i += 2 + k
        return out

    def items(self):
        for k in self.keys():              # (a snapshot of the keys: deleting while iterating is safe, as with a write cursor)
            v = self.get(k)
            if v is not None:
                yield k, v

    def close(self):
        if self._h:
            self._L.nbp_mdb_close(self._h)
            self._h = None

    def __del__(self):                     # (an environment dropped without close(): the file descriptor goes with it)
        try:
            self.close()
        except Exception:
            pass


def open_experience_db(path, map_size=200 * 1024 ** 3):
    """train_nbp_model.py:61-63.  The `lmdb` module when it is importable; otherwise LMDB's file format through the native container
    (MdbEnv) -- unless `path` already holds the append-only log of rounds 2-5 (data.log), which keeps opening as it was written."""
    try:
        import lmdb  # noqa: F401
        return LmdbEnv(path, map_size)
    except ImportError:
        pass
    if os.path.exists(os.path.join(path, "data.log")) and not os.path.exists(os.path.join(path, "data.mdb")):
        return LogEnv(path)
    return MdbEnv(path, map_size)


_last_key = [0]


def store_experience(env, data, replay_format="reference"):
    """ref :32-44.  The key is the millisecond clock; two records in the same millisecond would overwrite each
    other in the reference -- here the key is bumped so that none is lost."""
    store_packed(env, pack_record(data, replay_format))


def store_packed(env, value: bytes):
    """store_experience for a record already packed (pack_record)."""
    ms = max(int(time.time() * 1000), _last_key[0] + 1)
    _last_key[0] = ms
    env.put(f"{ms:012d}".encode(), value)


def store_validation_data(env, num=600 * 2, keep_compact=False):
    """ref :78-100: every ceil(total/num)-th record, up to `num`, is MOVED out of the store."""
    total = env.entries()
    print("Number of total data in the database:", total)
    n = max(math.ceil(total / num), 1)
    selected, delete_keys = [], []
    for count, (key, value) in enumerate(env.items()):
        if count % n == 0 and len(selected) < num:
            selected.append(unpack_record(value, keep_compact))
            delete_keys.append(key)
            if len(selected) == num:
                break
    for key in delete_keys:
        env.delete(key)
    return selected


def store_validation_data_readonly(env, num=600 * 2, keep_compact=False):
    """ref :46-61."""
    total = env.entries()
    n = max(math.ceil(total / num), 1)
    selected = []
    for count, (key, value) in enumerate(env.items()):
        if count % n == 0 and len(selected) < num:
            selected.append(unpack_record(value, keep_compact))
    return selected


def read_random_data_readonly(env, num_samples=64, keep_compact=False):
    """ref :63-76."""
    indices = set(random.sample(range(env.entries()), num_samples))
    return [unpack_record(v, keep_compact) for i, (k, v) in enumerate(env.items()) if i in indices]


def read_combined_data(env, sample_m=2304 * 2, sample_size=2176 * 2, keep_compact=False, with_keys=False):
    """ref :103-141: a random sample of the older records + the newest `sample_m` in order.  with_keys: every record also carries
    its store key as d["_key"] (what prioritised replay files a record's priority under); the default leaves the records as they are."""
    if with_keys:
        def unpack(key, value):
            d = unpack_record(value, keep_compact)
            d["_key"] = bytes(key)
            return d
        return _read_combined(env, sample_m, sample_size, unpack)
    return _read_combined(env, sample_m, sample_size, lambda key, value: unpack_record(value, keep_compact))


def _read_combined(env, sample_m, sample_size, unpack):
    total = env.entries()
    print("number of total data in the database:", total)
    if sample_m is None:
        return [unpack(k, v) for k, v in env.items()]
    n = total - sample_m
    if n < 0:
        n = 1
    sample_indices = set(random.sample(range(n), min(sample_size, n)))
    selected, tail = [], []
    first_tail = max(total - sample_m, 0)
    for i, (key, value) in enumerate(env.items()):
        if i < n and i in sample_indices:
            selected.append(unpack(key, value))
        if i >= first_tail:
            tail.append(unpack(key, value))
    return selected + tail


# ------------------------------------------------------------------ GT obstacle label
def get_binary_obstacle_array(mesh, camera_pose, view_size=80, grid_size=256, reference_label_semantics=True):
    """ref utils.py:226-262 -> [S,S] fp32 {0,1} on the device.  reference_label_semantics (default): the label sits on the pixel
    grid of the reference's matplotlib figure -- 80 units across the columns, 79.48 across the rows, 2.7-px strokes with projecting
    caps (hipops.reference_figure_geometry; pinned by tests/golden/obstacle_label.npz to within one pixel of line position).  False:
    the isotropic +-view_size/2 window at 1.04-px round strokes of rounds 1-5 (nbp_slice_obstacle_f32)."""
    x, y, z = (float(v) for v in list(camera_pose)[:3])
    if reference_label_semantics:
        return hipops.slice_obstacle_fig(mesh.verts, mesh.faces, y, x, z, grid_size, float(view_size))
    return hipops.slice_obstacle(mesh.verts, mesh.faces, y, x, z, grid_size, (-view_size / 2, view_size / 2))


# ------------------------------------------------------------------ trajectory collection
class CollectionRollout(lockstep.LockstepRollout):
    """One training rollout of trajectory_collection (ref :470-852) on one scene."""

    BETA = 0.5                     # Boltzmann temperature, ref :719
    P_RANDOM_HEADING = 0.6         # ref :768

    def __init__(self, params, nbp, camera, gt_scene_pc, mesh, y_bins, device, db_env, seed=0, grid=256,
                 value_size=64, grid_range=(-40, 40), replay_format="reference"):
        self.replay_format = check_replay_format(replay_format)
        self.params, self.nbp, self.camera, self.mesh, self.device, self.db = params, nbp, camera, mesh, device, db_env
        self.y_bins, self.S, self.V, self.grid_range = y_bins, grid, value_size, grid_range
        self.st = lockstep.RolloutState(device, grid=grid)         # (depth only, maps without bins: st.bins stays None)
        self.rng = random.Random(seed)
        self.planner = LatticePlanner(camera, mesh, device, value_size, grid, grid_range, rng=self.rng)
        self.gt = gt_scene_pc.contiguous()
        self.bbox = (self.gt.min(0).values.tolist(), self.gt.max(0).values.tolist())
        self.cov_plan = hipops.CoveragePlan(self.gt, 1.0, 2, self.bbox)
        self.gen = torch.Generator().manual_seed(seed)
        self.step_seed = seed * 1_000_003
        self.pose_i = 0
        # check_camera_in_mesh for every lattice position, once per scene (static mesh)
        cnt = hipops.axis_ray_counts(mesh.verts, mesh.faces, self.planner.pos_dev).cpu().numpy()
        self.inside = np.all(cnt % 2 == 1, axis=1)
        self.edge_ok = ~self.planner.mesh_hit.astype(bool)             # training_flag branch of get_neighbors
        self.path, self.path_record = [], 0
        self.unreachable = set()
        self.experiences = []
        self.coverage_evolution = []
        self.coverage_at_trajectory = None
        self.n_stored = 0
        lockstep._settle_gc()                   # the planner's long-lived tables leave the cyclic collector's walks (see there)

    # -- The step in four phases -- observe, inputs, decide, move -- each a GPU half and a host half.  run() composes them for this
    # rollout alone; CollectionGroup runs the GPU halves of a lock-step group as group launches and calls the same host halves.
    def _observe(self):
        """S1-S4: coverage of the cloud so far (GPU half + the host half `_observed`)."""
        return self._coverage(self.count_coverage()[0].item())

    def _coverage(self, count):
        return float(np.float32(count) / np.float32(len(self.gt)))

    def _observed(self, pose_i, cov):
        """Host half of observe: records the coverage; True when the rollout is done (coverage > 0.95)."""
        self.coverage_evolution.append(cov)
        if pose_i == getattr(self.params, "n_poses_in_trajectory", -1):
            self.coverage_at_trajectory = cov
        return cov > 0.95

    def _inputs(self):
        """S5-S8: current frame, maps, trajectory image, GT label -> (pose, model_input [1,5,S,S], gt_obs [1,1,S,S])."""
        st, cam = self.st, self.camera
        self.unproject(lockstep.CURRENT, False)
        pose = cam.pose_from_idx(cam.cam_idx)
        hu.accumulate_step_maps(st.cloud, pose, self.y_bins, self.S, self.grid_range, n_dev=st.cloud_count, out=st.maps6)
        traj2d = hu.transform_points_to_n_pieces(cam.trajectory_points(), pose)
        traj_img = hu.map_points_to_n_imgs(traj2d, (self.S, self.S), self.grid_range)
        model_input = torch.cat((st.maps6[:4], traj_img), 0).unsqueeze(0).clone()
        gt_obs = get_binary_obstacle_array(self.mesh, pose, self.grid_range[1] * 2, self.S).reshape(1, 1, self.S, self.S)
        return pose, model_input, gt_obs

    def label_item(self, pose):
        x, y, z = (float(v) for v in list(pose)[:3])
        return (self.mesh.verts, self.mesh.faces, y, x, z)

    def _needs_replan(self):
        return self.path is not None and self.path_record + 1 > len(self.path)

    def _decide_begin(self, pose_i, cells=None):
        """Host half of decide, before the goal scores: flush the finished segment (cells: its hindsight cells from the group
        launch, None: computed here) and start a new path."""
        if self.experiences:
            self._flush_experiences(pose_i, cells)
        self.path_record = 0

    def _decide_end(self, cov, pose, model_input, gt_obs):
        """Host half of decide, after any replan: keeps the experience; True when the rollout is done (no path)."""
        if self.path is None or len(self.path) == 0:
            return True
        self.experiences.append([cov, model_input, gt_obs, list(pose), int(self.camera.cam_idx[4])])
        return self.path_record >= len(self.path)

    def _next_idx(self):
        """Host half of move: the next lattice pose (60 % random heading)."""
        next_idx = list(self.path[self.path_record])
        if self.rng.random() <= self.P_RANDOM_HEADING:
            next_idx[4] = self.rng.randrange(8)
        return next_idx

    def _move(self):
        """S10-S14: move (4 poses, one raster launch), un-project the supervision frames."""
        self.camera.move_and_capture(self.mesh, self._next_idx())
        self.unproject(lockstep.SUPERVISION, False)
        self.path_record += 1

    def hindsight_xz(self):
        """(x, z) of the finished segment's poses, fp32 as transform_points_to_n_pieces reads them."""
        return np.asarray([[e[3][0], e[3][2]] for e in self.experiences], np.float32).reshape(-1, 2)

    def _flush_experiences(self, pose_i, cells=None):
        """Hindsight relabelling (ref :655-693): every later pose of the finished path that falls inside the
        value map of an earlier one becomes a target pixel (its heading, its cell) with the coverage gained.
        cells: host [m,m] int32 from hipops.hindsight_cells_batch (row * V + col, -1 outside); None: per experience here."""
        ex_list = self.experiences
        for a in range(len(ex_list)):
            later = ex_list[a + 1:]
            if not later:
                continue
            if cells is None:
                pts = torch.tensor([list(e[3][:3]) for e in later], dtype=torch.float32, device=self.device)
                p2d = hu.transform_points_to_n_pieces(pts, ex_list[a][3])
                rc = hu.get_point_position_in_the_img(p2d.squeeze(0), (self.V, self.V), self.grid_range)
                rc = rc.reshape(2, -1).cpu().numpy()
            else:
                row = cells[a, a + 1:]
                rc = np.stack([np.where(row >= 0, row // self.V, -1), np.where(row >= 0, row % self.V, -1)])
            pixels, gains = [], []
            for j, e in enumerate(later):
                r, c = int(rc[0, j]), int(rc[1, j])
                if 0 <= r < self.V and 0 <= c < self.V:
                    d = e[0] - ex_list[a][0]
                    pixels.append([int(e[4]), r, c])
                    gains.append(d * 100 if d > 0 else 0)
            if pixels:
                # (compact collection: the experience holds its encoded slot, no label -- pack_record keeps the stream's bytes)
                images = ({"nbpc": ex_list[a][1]} if ex_list[a][2] is None else
                          {"current_model_input": ex_list[a][1], "current_gt_2d_layout": ex_list[a][2]})
                self.put({
                    **images,
                    "target_value_map_pixel": np.asarray(pixels, np.int64),
                    "actual_coverage_gain": np.asarray(gains, np.float32), "pose_i": pose_i})
                self.n_stored += 1
        self.experiences = []

    def put(self, data):
        store_experience(self.db, data, self.replay_format)

    def _replan(self, pose, model_input):
        """Boltzmann goal sampling + search (ref :695-745).  Returns the path or None."""
        pl = self.planner
        with torch.no_grad():
            out1, _ = self.nbp(model_input)
        o1 = out1[0]
        p2d = hu.transform_points_to_n_pieces(pl.pos_dev, pose)
        cells = hu.get_point_position_in_the_img(p2d.squeeze(0), (self.V, self.V), self.grid_range).reshape(2, -1)
        max_gain = o1.amax(0)
        ok = (cells[0] >= 0) & (cells[0] < self.V) & (cells[1] >= 0) & (cells[1] < self.V)
        vals = max_gain[cells[0].clamp(0, self.V - 1), cells[1].clamp(0, self.V - 1)]
        return self._search(pose, ok.cpu().numpy(), vals.cpu().numpy(), o1.cpu().numpy())

    def _search(self, pose, ok_h, vals_h, out1_h):
        """Host half of the replan: Boltzmann draw over the in-window candidates, then the search (own rng / generator)."""
        pl, cam = self.planner, self.camera
        start_id = pl.node_index[tuple(cam.cam_idx[:3])]
        cand = [n for n in range(len(pl.idx3)) if ok_h[n] and n != start_id]
        if not cand:
            return None
        probs = torch.softmax(torch.from_numpy(vals_h[cand]).double() / self.BETA, 0)
        first = int(torch.multinomial(probs, 1, generator=self.gen).item())
        cand.insert(0, cand.pop(first))
        tree = planner_host.level_order_tree(pl.nbrs, self.edge_ok, start_id)
        hist = np.asarray(cam.cam_idx_history, np.int64).reshape(-1, 5)
        for n in cand:
            if not self.inside[n] or n in self.unreachable:
                continue
            if n not in tree:
                self.unreachable.add(n)
                continue
            ids, cur = [], n
            while cur >= 0:
                ids.append(cur)
                cur = tree[cur]
            nodes = [tuple(pl.idx3[m].tolist()) for m in ids[::-1]]
            full = planner_host.choose_headings(nodes, pl.xyz, pl.node_index, pose, out1_h, hist, self.V, self.grid_range,
                                                rng=self.rng)
            return full[1:]
        return None

    def run(self, n_poses=100, coverage_after_trajectory=None):
        for pose_i in range(n_poses):
            self.pose_i = pose_i
            done = self._observed(pose_i, self._observe())
            if coverage_after_trajectory is not None and self.coverage_at_trajectory is not None:
                coverage_after_trajectory.append(self.coverage_at_trajectory)
                self.coverage_at_trajectory = None
            if done:
                break
            pose, model_input, gt_obs = self._inputs()
            if self._needs_replan():
                self._decide_begin(pose_i)
                self.path = self._replan(pose, model_input)
            if self.replay_format == "compact":     # the record's planes through the encoder, one record: the experience keeps the slot
                model_input, gt_obs = hipops.replay_encode(torch.cat((model_input, gt_obs), 1))[0], None
            if self._decide_end(self.coverage_evolution[-1], pose, model_input, gt_obs):
                break
            self._move()
        return self.coverage_evolution


class CollectionGroup:
    """Up to K CollectionRollouts of one rank in lock-step (trajectory_collection(..., rollouts_per_gpu=K)).  Every phase of the
    step runs once per group step for the live rollouts: coverage (one group launch, one read-back of K counts), the current frame's
    un-projection, the maps + trajectory channel, the GT label, ONE forward of the replanning rollouts' inputs, their goal scores
    (one launch, one read-back with the out1 rows), the hindsight cells of the flushing rollouts (one launch, one read-back), the
    move's render and the supervision frames' un-projection -- each a group launch.  The host halves are CollectionRollout's own
    (each rollout keeps its random.Random and torch.Generator, so the draws are the serial run's).  A rollout that finishes leaves
    and its slot takes the rank's next scene.  Records are packed per scene and reach the store in serial order: scene order, then
    flush order within a scene (the earliest unfinished scene streams its records; later scenes hold theirs until it is done)."""

    def __init__(self, make_rollout, scenes, K, n_poses, device, timing=None, replay_format="reference"):
        self.make, self.queue, self.K, self.n_poses, self.device = make_rollout, list(scenes), int(K), n_poses, device
        self.replay_format = check_replay_format(replay_format)
        self.order = list(scenes)                  # commit order
        self.held = {si: [] for si in self.order}  # packed records not yet in the store
        self.done = {}                             # si -> finished rollout's (coverage_at_trajectory, n_stored)
        self.live = []                             # [(si, rollout)]
        self.t = timing if timing is not None else {}
        self.n_poses_done = 0
        self.stored = 0
        self._buf = None

    def _tick(self, key, t0):
        t1 = time.perf_counter()
        self.t[key] = self.t.get(key, 0.0) + (t1 - t0)
        return t1

    def _refill(self):
        t0 = time.perf_counter()
        while len(self.live) < self.K and self.queue:
            si = self.queue.pop(0)
            ro = self.make(si)
            held = self.held[si]
            ro.put = lambda data, held=held: held.append(data)       # packed in one place per group step (_pack)
            self.live.append((si, ro))
        self._tick("setup_s", t0)

    def _leave(self, si, ro):
        self.done[si] = (ro.coverage_at_trajectory, ro.n_stored)

    def _commit(self, db, coverage_after_trajectory):
        """Records into the store in serial order (the first scene of `order` is the only one that may write)."""
        t0 = time.perf_counter()
        while self.order:
            si = self.order[0]
            for value in self.held[si]:
                store_packed(db, value)
            self.held[si].clear()
            if si not in self.done:
                break
            cov_t, n = self.done.pop(si)
            if coverage_after_trajectory is not None and cov_t is not None:
                coverage_after_trajectory.append(cov_t)
            self.stored += n
            del self.held[si]
            self.order.pop(0)
        self._tick("store_put_s", t0)

    def _pack(self):
        t0 = time.perf_counter()
        for held in self.held.values():             # in place: the rollouts' put() appends to these lists
            held[:] = [v if isinstance(v, bytes) else pack_record(v, self.replay_format) for v in held]
        self._tick("pack_s", t0)

    def _buffers(self, n, S):
        if self._buf is None or self._buf[0].shape[0] < n:
            K = max(n, self.K)
            self._buf = (torch.zeros(K, 6, S, S, dtype=torch.float32, device=self.device),
                         torch.zeros(K, 5, S, S, dtype=torch.float32, device=self.device))
        return self._buf[0][:n], self._buf[1][:n]

    def run(self, db, coverage_after_trajectory=None):
        self._refill()
        while self.live:
            self.step()
            self._pack()
            self._commit(db, coverage_after_trajectory)
            if len(self.live) < self.K and self.queue:
                torch.cuda.empty_cache()
                self._refill()
        self._commit(db, coverage_after_trajectory)
        return self.stored

    def _drop(self, keep):
        keep_ids = {id(ro) for ro in keep}
        for si, ro in self.live:
            if id(ro) not in keep_ids:
                self._leave(si, ro)
        self.live = [(si, ro) for si, ro in self.live if id(ro) in keep_ids]

    def step(self):
        t0 = time.perf_counter()
        grp = [ro for _, ro in self.live]
        r0 = grp[0]
        S, V, gr = r0.S, r0.V, r0.grid_range
        # -- observe: coverage in one group launch, one read-back of the counts
        hipops.coverage_count_batch([ro.coverage_item() for ro in grp])
        counts = torch.stack([ro.st.coverage_counts[ro.pose_i % ro.st.coverage_counts.shape[0], 0] for ro in grp]).cpu().tolist()
        t0 = self._tick("gpu_step_s", t0)
        covs = {}
        alive = []
        for ro, c in zip(grp, counts):
            cov = ro._coverage(c)
            if not ro._observed(ro.pose_i, cov):
                covs[id(ro)] = cov
                alive.append(ro)
        self.n_poses_done += len(grp)
        self._drop(alive)
        grp = alive
        if not grp:
            return
        t0 = self._tick("host_search_s", t0)
        # -- inputs: the current frame, the maps + trajectory channel, the label
        lockstep.unproject_group(grp, lockstep.CURRENT, False)
        n = len(grp)
        maps6, net_in = self._buffers(n, S)
        hu.step_maps_batch([ro.maps_item() for ro in grp], S, gr, maps6, net_in)
        poses = [ro.pose for ro in grp]
        label = hipops.slice_obstacle_fig_batch([ro.label_item(pose) for ro, pose in zip(grp, poses)], S, float(gr[1] * 2))
        rec = torch.empty(n, 6, S, S, dtype=torch.float32, device=self.device)
        rec[:, :5].copy_(net_in)
        rec[:, 5].copy_(label)
        # the records' tensors: one copy per group step (complete before any flush reads them: a flush happens in a later group step,
        # after that step's blocking read-back of the coverage counts on this stream)
        # (compact records: the step's planes through the encoder first -- two more launches on this stream, no synchronisation --
        # and the copy moves the arena of streams instead; an experience keeps its slot, the flush keeps the stream's total_bytes)
        compact = self.replay_format == "compact"
        src = hipops.replay_encode(rec) if compact else rec
        rec_h = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
        rec_h.copy_(src, non_blocking=True)
        # -- decide: flush the finished segments (hindsight cells in one launch), ONE forward of the replanning rollouts' inputs
        replan = [i for i, ro in enumerate(grp) if ro._needs_replan()]
        flush = [i for i in replan if len(grp[i].experiences) > 1]
        cells_h = {}
        if flush:
            xz = [grp[i].hindsight_xz() for i in flush]
            xz_dev = torch.from_numpy(np.concatenate(xz)).to(self.device)
            sizes = [len(a) ** 2 for a in xz]
            cells_dev = torch.empty(sum(sizes), dtype=torch.int32, device=self.device)
            offs = np.concatenate([[0], np.cumsum([len(a) for a in xz])]).tolist()
            coffs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
            hipops.hindsight_cells_batch([(xz_dev[offs[k]:offs[k + 1]], cells_dev[coffs[k]:coffs[k + 1]]) for k in range(len(flush))],
                                         V, gr)
            allc = cells_dev.cpu().numpy()
            for k, i in enumerate(flush):
                m = len(xz[k])
                cells_h[i] = allc[coffs[k]:coffs[k + 1]].reshape(m, m)
        goal = {}
        if replan:
            x = net_in if len(replan) == n else net_in[torch.tensor(replan, device=self.device)]
            with torch.no_grad():
                out1, _ = grp[0].nbp(x)
            B = len(replan)
            P = max(grp[i].planner.pos_dev.shape[0] for i in replan)
            VV8 = 8 * V * V
            G = torch.empty(B, 2 * P + VV8, dtype=torch.float32, device=self.device)
            gitems = []
            for b, i in enumerate(replan):
                ro = grp[i]
                pos = ro.__dict__.get("_pos32")
                if pos is None:
                    pos = ro._pos32 = ro.planner.pos_dev.float().contiguous()
                Pi = pos.shape[0]
                gitems.append((pos, (float(poses[i][0]), float(poses[i][2])), out1[b].reshape(8, V, V).contiguous(),
                               G[b, P:P + Pi].view(torch.int32), G[b, :Pi]))
            hipops.goal_values_batch(gitems, V, gr)
            G[:, 2 * P:].copy_(out1.reshape(B, VV8))
            Gh = G.cpu()
            for b, i in enumerate(replan):
                Pi = gitems[b][0].shape[0]
                cell = Gh[b, P:P + Pi].view(torch.int32).numpy()
                goal[i] = (cell >= 0, Gh[b, :Pi].numpy(), Gh[b, 2 * P:].reshape(8, V, V).numpy())
        t0 = self._tick("gpu_step_s", t0)
        alive = []
        for i, ro in enumerate(grp):
            model_input, gt_obs = (rec_h[i], None) if compact else (rec_h[i:i + 1, :5], rec_h[i:i + 1, 5:6])
            if i in goal:
                ro._decide_begin(ro.pose_i, cells_h.get(i))
                ro.path = ro._search(poses[i], *goal[i])
            if not ro._decide_end(covs[id(ro)], poses[i], model_input, gt_obs):
                alive.append(ro)
        t0 = self._tick("host_search_s", t0)
        # -- move: the render in one group launch, the supervision frames' un-projection in one
        self._drop(alive)
        grp = alive
        if not grp:
            return
        next_idx = [ro._next_idx() for ro in grp]
        t0 = self._tick("host_search_s", t0)
        lockstep.render_moves(grp, next_idx)
        lockstep.unproject_group(grp, lockstep.SUPERVISION, False)
        alive = []
        for ro in grp:
            ro.path_record += 1
            ro.pose_i += 1
            if ro.pose_i < self.n_poses:
                alive.append(ro)
        self._drop(alive)
        self._tick("gpu_step_s", t0)


def trajectory_collection(params, current_epoch, dataset, db_env, pc2img_size, value_map_size, prediction_range, nbp,
                          coverage_after_trajectory, memory, device, folder_img_path=None, rank=0, world=1, n_poses=100,
                          n_gt_points=None, rollouts_per_gpu=1, timing=None, replay_format=None, depth_noise=None,
                          depth_filter=None):
    """ref :470-852.  `dataset` is a simulator.scene.SceneDataset; with world > 1 each rank collects the scenes
    rank, rank + world, ... into its own store (collection is embarrassingly parallel).
    rollouts_per_gpu = K > 1: up to K of the rank's scenes in lock-step (CollectionGroup); the store receives the same records in
    the same order as with K = 1.  `timing` (a dict, K > 1) receives the seconds of the group's stages.
    replay_format: "reference" (the reference's record bytes) or "compact" (utility/replay_codec.py: the same record, its images
    encoded on the device before they leave it); None = params.replay_format, "reference" when the config does not name one.
    depth_noise: the cameras' sensor model (utility/depth_noise.py::option_spec; None = off, perfect depth): what the collecting policy
    sees and un-projects is the noisy depth, while the labels, slices of the mesh, do not change.
    depth_filter: the cameras' frame filter behind the sensor (utility/depth_filter.py::option_spec; None = off); the labels do not
    change with it either."""
    nbp.eval()
    from .depth_filter import option_spec as filter_option_spec
    from .depth_noise import option_spec
    noise_spec = option_spec(depth_noise)
    filter_spec = filter_option_spec(depth_filter)
    replay_format = check_replay_format(getattr(params, "replay_format", "reference") if replay_format is None else replay_format)

    def make(si):
        sd = dataset[si]
        settings = sim_scene.Settings(sd["settings"], params.scene_scale_factor)
        mesh = sim_scene.load_scene(os.path.join(dataset.data_path, sd["scene_name"], sd["obj_name"]),
                                    params.scene_scale_factor, device)
        y_bins = sim_scene.y_bins_for(mesh.verts_host, 4)
        seed = 7919 * current_epoch + si
        _, gt_dev = sim_scene.setup_gt_scene(params, settings, mesh, device, 0.05, seed=seed, n_points=n_gt_points)
        camera = lockstep.setup_test_camera(params, mesh, settings.camera.start_positions[0], settings, device, seed=seed,
                                            depth_noise=noise_spec, depth_filter=filter_spec)
        return CollectionRollout(params, nbp, camera, gt_dev, mesh, y_bins, device, db_env, seed,
                                 pc2img_size[0], value_map_size[0], prediction_range, replay_format=replay_format)

    scenes = list(range(rank, len(dataset), world))
    if int(rollouts_per_gpu) > 1:
        return CollectionGroup(make, scenes, rollouts_per_gpu, n_poses, device, timing, replay_format).run(db_env,
                                                                                                           coverage_after_trajectory)
    stored = 0
    for si in scenes:
        ro = make(si)
        ro.run(n_poses, coverage_after_trajectory)
        stored += ro.n_stored
        del ro
        torch.cuda.empty_cache()
    return stored

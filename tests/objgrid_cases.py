"""The scenes of tests/test_objgrid_cpu.py and tests/test_gpu_objgrid.py (no test in here): objects as (vertices, faces)
in world coordinates, their oracle tests/mesh_iou_f64.voxelize and their restatement tests/objgrid_ref.restate, each
computed once per (object, voxel size) and never changed afterwards.  The vertices are what a SceneMesh holds: float32."""
import functools

import numpy as np

import mesh_iou_f64 as M
import objgrid_ref as G
import simplify_cases as SC

# the pieces of ragged_scene() of tests/test_gpu_mesh_eval.py
CUBE_V = np.array([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)])
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]])
TETRA_V = np.array([[0., 0., 0.], [0.8, 0.1, 0.05], [0.2, 0.7, 0.1], [0.3, 0.25, 0.6]])
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
NO_V, NO_F = np.zeros((0, 3)), np.zeros((0, 3), np.int64)

FEW_SIZES = (0.5, 1 / 7.5, 1 / 63.5, 1 / 64.5, 1 / 65.5, 1 / 129.5)      # the cube: D = 2, 7, 63, 64, 65, 129
MANY_SIZES = (1 / 20.5, 1 / 33.5)


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def _objects():
    tetra = TETRA_V + [0.6, -1.0, 2.1]
    flat = tetra.copy()
    flat[:, 2] = 2.1
    few = [("empty", NO_V, NO_F),
           ("cube", CUBE_V * [1.0, 0.7, 0.4] + [0.3, -1.2, 2.0], CUBE_F),
           ("tetrahedron", tetra, TETRA_F),
           ("nan", np.full((3, 3), np.nan), np.array([[0, 1, 2]])),
           ("doubled", tetra, np.concatenate([TETRA_F[:1], TETRA_F])),            # face 0 twice: I comes out empty
           ("open", tetra, TETRA_F[:-1]),
           ("degenerate", tetra, np.concatenate([TETRA_F, [[0, 0, 1]]])),
           ("flat", flat, TETRA_F),                                               # S without I
           ("empty_last", NO_V, NO_F)]
    many = [("icosphere2", *SC.icosphere(2)), ("icosphere3", *SC.icosphere(3)), ("torus", *SC.torus()),
            ("patch", *SC.patch())]
    # as they come, about the origin: the torus' lattice centres then fall exactly on triangle edges
    return {n: (_f32(v), np.asarray(f, np.int64).reshape(-1, 3)) for n, v, f in few + many}, \
        [n for n, _, _ in few], [n for n, _, _ in many]


OBJECTS, FEW, MANY = _objects()


def objects(names):
    return [OBJECTS[n] for n in names]


@functools.lru_cache(maxsize=None)
def oracle(name, voxel_size):
    """tests/mesh_iou_f64.voxelize -> M.Obj (U None: no grid)"""
    v, f = OBJECTS[name]
    if len(v) == 0:
        return M.Obj()
    with np.errstate(divide='ignore', invalid='ignore'):      # the flat object: C1 divides by zero, nothing is a candidate
        return M.voxelize(v, f, voxel_size)


@functools.lru_cache(maxsize=None)
def restated(name, voxel_size):
    v, f = OBJECTS[name]
    return G.restate(v, f, voxel_size) if len(v) else G.Restated()


def oracle_batch(names, voxel_size):
    """the ObjectGrids of the oracle as numpy: dims, off, frame, cnt, words (uint64)"""
    objs = [oracle(n, voxel_size) for n in names]
    N = len(objs)
    dims, off, frame, cnt = np.zeros(N, np.int32), np.zeros(N, np.int64), np.zeros((N, 4)), np.zeros((N, 2), np.int32)
    packed, total = [], 0
    for k, o in enumerate(objs):
        if o.U is None:
            continue
        w = M.pack_words(o.U)
        dims[k], off[k] = o.S.shape[0], total
        frame[k, :3], frame[k, 3] = o.lo, o.cell
        cnt[k] = int(o.U.sum()), int(o.S.sum())
        packed.append(w)
        total += len(w)
    words = np.concatenate(packed) if packed else np.zeros(1, np.uint64)
    return {"dims": dims, "off": off, "frame": frame, "cnt": cnt, "words": words}


def scene_mesh(objs, device):
    """[(vertices, faces)] -> SceneMesh on `device`, built as scene.place_in_corners lays one out"""
    import torch
    from rfdnet_amd.iscnet.scene import SceneMesh
    obj_off = np.concatenate([[0], np.cumsum([len(v) for v, _ in objs])]).astype(np.int64)
    face_off = np.concatenate([[0], np.cumsum([len(f) for _, f in objs])]).astype(np.int64)
    v = np.concatenate([v for v, _ in objs] + [NO_V]).astype(np.float32)
    f = np.concatenate([f + o for (_, f), o in zip(objs, obj_off)] + [NO_F]).astype(np.int32)
    face_obj = np.repeat(np.arange(len(objs)), np.diff(face_off)).astype(np.int32)
    t = lambda a: torch.from_numpy(a).to(device)
    return SceneMesh(vertices=t(v), faces=t(f), face_obj=t(face_obj), obj_off=t(obj_off.astype(np.int32)),
                     face_off=t(face_off.astype(np.int32)), obj_class=torch.zeros(len(objs), dtype=torch.int32, device=device),
                     normals=None)


def grids_as_numpy(g):
    """ObjectGrids -> the same dict as oracle_batch"""
    return {"dims": g.dim.cpu().numpy(), "off": g.off.cpu().numpy(), "frame": g.frame.cpu().numpy(),
            "cnt": g.cnt.cpu().numpy(), "words": g.words.cpu().numpy().view(np.uint64)}


def assert_same_grids(got, want):
    for k in ("dims", "off", "frame", "cnt", "words"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), k

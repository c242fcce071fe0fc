"""Input / output formats of the demo path.

  read_off            the scan format of demo/inputs/*.off (trimesh.load(...).vertices,
                      demo.py:25)
  write_off           the format of the watertight CAD meshes (mcubes.export_off in
                      utils/shapenet/1_fuse_shapenetv2.py); read_off reads it back
  read_obj            ShapeNet's model_normalized.obj: `v` and `f` records
  read_mesh           "a mesh file" of the mesh tools: .off, .obj or .ply -> float64 vertices, int32 triangles
  write_binvox        `#binvox 1` voxel grids as the reference's external/binvox_rw.py writes them
  read_binvox         (axis order xyz, run-length pairs); write_points_npz / write_pointcloud_npz:
                      points.npz and pointcloud.npz of utils/shapenet/2_sample_mesh.py;
                      read_pointcloud_npz reads the latter back
  load_demo_data      demo.py:24-48: vertices -> [xyz | height] -> random_sampling
                      (utils/pc_util.py:35-47) -> (1, N, 4) float32 tensor
  write_mesh_ply      `proposal_%d_mesh.ply` as trimesh exports it (binary
                      little-endian, float xyz, `list uchar int` faces; header of
                      demo/outputs/scene0549_00/proposal_22_mesh.ply)
  write_points_ply    `%06d_pc.ply` (pc_util.write_ply)
  save_visualization  demo.py:278-327: meshes + `%06d_pred_confident_nms_bbox.npz`
                      with obbs (K,7) and proposal_map (K,1)
  write_png           8-bit RGB, no interlace, by zlib and struct alone
  save_scene          what the reference's `visualize` shows (demo.py:329-377), as files: the
                      placed objects in one mesh `scene_objects.ply` and the picture `pred.png`
"""
import os
import struct
import zlib

import numpy as np


def read_off(path):
    """-> (vertices (V,3+) float64, faces list).  Handles 'OFF' and 'COFF'
    headers and the 'OFF<counts>' single-line variant."""
    with open(path, "r") as f:
        tokens = f.read().split()
    head = tokens[0]
    pos = 1
    if head not in ("OFF", "COFF", "NOFF"):
        if head.startswith("OFF") and head[3:].isdigit():
            tokens = ["OFF", head[3:]] + tokens[1:]
        else:
            raise ValueError("not an OFF file: %s" % path)
    nv, nf = int(tokens[pos]), int(tokens[pos + 1])
    pos += 3
    rest = tokens[pos:]
    # vertex rows may carry colours: infer the row width from the face section
    faces = []
    width = 3
    for cand in (3, 6, 7):
        if nv * cand <= len(rest):
            p = nv * cand
            ok = True
            for _ in range(min(nf, 8)):
                if p >= len(rest):
                    ok = False
                    break
                k = int(float(rest[p]))
                if k < 1 or k > 64:
                    ok = False
                    break
                p += 1 + k
            if ok:
                width = cand
                break
    v = np.array(rest[:nv * width], dtype=np.float64).reshape(nv, width)
    p = nv * width
    for _ in range(nf):
        k = int(rest[p])
        faces.append([int(x) for x in rest[p + 1:p + 1 + k]])
        p += 1 + k
        # optional per-face colour values are not consumed (unused on this path)
    return v, faces


def write_off(path, vertices, faces):
    """vertices (V,3), faces (F,k) or a list of index lists -> an 'OFF' file that read_off reads back (17 significant
    digits: a float64 survives the round trip)"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    faces = [[int(i) for i in f] for f in (faces.tolist() if hasattr(faces, "tolist") else faces)]
    lines = ["OFF", "%d %d 0" % (v.shape[0], len(faces))]
    lines += ["%.17g %.17g %.17g" % (p[0], p[1], p[2]) for p in v]
    lines += [" ".join(str(i) for i in [len(f)] + f) for f in faces]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def read_obj(path):
    """-> (vertices (V,3) float64, faces (F,3) int32) of a Wavefront OBJ: `v` and `f` records only (the reference reads
    ShapeNet's models with flags=('v', 'f')); a face token may be a, a/b, a//c or a/b/c (the vertex index counts), a
    polygon is fanned into triangles from its first corner.  A negative (relative) or out-of-range index is refused."""
    vertices, faces = [], []
    with open(path, "r") as fh:
        for number, line in enumerate(fh, 1):
            rec = line.split("#", 1)[0].split()
            if not rec:
                continue
            if rec[0] == "v":
                if len(rec) < 4:
                    raise ValueError("%s:%d: a vertex has three coordinates" % (path, number))
                vertices.append([float(t) for t in rec[1:4]])
            elif rec[0] == "f":
                idx = [int(t.split("/")[0]) for t in rec[1:]]
                if len(idx) < 3:
                    raise ValueError("%s:%d: a face has at least three corners" % (path, number))
                if min(idx) < 1:
                    raise ValueError("%s:%d: negative (relative) and zero indices are not supported" % (path, number))
                faces += [[idx[0] - 1, idx[k] - 1, idx[k + 1] - 1] for k in range(1, len(idx) - 1)]
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and f.max() >= v.shape[0]:
        raise ValueError("%s: a face names vertex %d of %d" % (path, f.max() + 1, v.shape[0]))
    return v, f.astype(np.int32)


def write_binvox(path, voxels, translate, scale):
    """voxels (R,R,R) bool indexed [x, y, z] -> a '#binvox 1' file as the reference's binvox_rw writes it for
    axis_order='xyz': the file's own order is x, z, y (y fastest), run-length pairs (value, count) with count <= 255.
    Byte for byte binvox_rw's, including its one quirk: a run whose length is a multiple of 255 and that is not the last
    ends with a pair of count 0 (which every reader skips)."""
    v = np.asarray(voxels)
    if v.ndim != 3 or v.size == 0:
        raise ValueError("write_binvox: a non-empty (X,Y,Z) grid, got %s" % (v.shape,))
    flat = np.transpose(v.astype(bool), (0, 2, 1)).reshape(-1).astype(np.uint8)
    start = np.concatenate([[0], np.nonzero(np.diff(flat))[0] + 1])
    length = np.diff(np.concatenate([start, [flat.size]]))
    pairs = bytearray()
    for i, (value, n) in enumerate(zip(flat[start].tolist(), length.tolist())):
        pairs += bytes([value, 255]) * (n // 255)
        if n % 255 or i + 1 < len(start):
            pairs += bytes([value, n % 255])
    head = "#binvox 1\ndim %s\ntranslate %s\nscale %s\ndata\n" % (
        " ".join(str(int(d)) for d in v.shape), " ".join(str(float(t)) for t in np.asarray(translate).reshape(-1)),
        str(float(scale)))
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii") + bytes(pairs))


def read_binvox(path):
    """-> (voxels (X,Y,Z) bool indexed [x, y, z], translate (3,) float64, scale float) of a '#binvox 1' file"""
    with open(path, "rb") as fh:
        if not fh.readline().strip().startswith(b"#binvox"):
            raise ValueError("not a binvox file: %s" % path)
        dims = [int(t) for t in fh.readline().split()[1:]]
        translate = np.array([float(t) for t in fh.readline().split()[1:]], np.float64)
        scale = float(fh.readline().split()[1])
        fh.readline()
        raw = np.frombuffer(fh.read(), np.uint8)
    flat = np.repeat(raw[::2], raw[1::2]).astype(bool)
    if len(dims) != 3 or flat.size != int(np.prod(dims)):
        raise ValueError("%s: %d voxels in the runs, dim %s" % (path, flat.size, dims))
    return np.transpose(flat.reshape(dims[0], dims[2], dims[1]), (0, 2, 1)).copy(), translate, scale


def _npz_arrays(points, loc, scale, float16):
    return (np.asarray(points).astype(np.float16 if float16 else np.float32), np.asarray(loc, np.float64),
            np.float64(scale))


def write_points_npz(path, points, occupancies, loc, scale, float16=False, packbits=False):
    """The reference's points.npz (export_points): points (n,3) f32 or f16, occupancies (n,) bool or, with packbits,
    the uint8 of np.packbits, loc (3,), scale"""
    points, loc, scale = _npz_arrays(points, loc, scale, float16)
    occ = np.asarray(occupancies).astype(bool)
    np.savez(path, points=points, occupancies=np.packbits(occ) if packbits else occ, loc=loc, scale=scale)


def write_pointcloud_npz(path, points, normals, loc, scale, float16=False, packbits=False):
    """The reference's pointcloud.npz (export_pointcloud): points and normals (n,3) f32 or f16, loc (3,), scale.  There is
    nothing boolean in it: packbits is accepted for symmetry with write_points_npz and changes nothing."""
    points, loc, scale = _npz_arrays(points, loc, scale, float16)
    np.savez(path, points=points, normals=np.asarray(normals).astype(points.dtype), loc=loc, scale=scale)


def read_pointcloud_npz(path, original_frame=False):
    """The inverse of write_pointcloud_npz -> points (n,3), normals (n,3), loc (3,) f64, scale (float).  Points and normals
    come back as float32 (a float16 file is upcast, which is exact).  The file's points are in the unit cube of
    tools/sample_mesh.py, p = (x - loc) / scale; original_frame=True returns x = p scale + loc in float64 instead (the
    normals are directions and stay)."""
    with np.load(path) as z:
        missing = [k for k in ("points", "normals") if k not in z.files]
        if missing:
            raise ValueError("%s: no %s (a pointcloud.npz holds points, normals, loc, scale)" % (path, ", ".join(missing)))
        points, normals = z["points"], z["normals"]
        loc = np.asarray(z["loc"], np.float64).reshape(3) if "loc" in z.files else np.zeros(3)
        scale = float(z["scale"]) if "scale" in z.files else 1.
    if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
        raise ValueError("%s: points %s and normals %s are not two (n,3) arrays" % (path, points.shape, normals.shape))
    if points.dtype not in (np.float16, np.float32) or normals.dtype not in (np.float16, np.float32):
        raise ValueError("%s: points are %s, normals %s: float16 or float32 expected" % (path, points.dtype, normals.dtype))
    points, normals = points.astype(np.float32), normals.astype(np.float32)
    if original_frame:
        points = points.astype(np.float64) * scale + loc
    return points, normals, loc, scale


def random_sampling(pc, num_sample, rng, replace=None):
    """utils/pc_util.py:35-47 (with replacement iff the scan has fewer points)."""
    if replace is None:
        replace = pc.shape[0] < num_sample
    choices = rng.choice(pc.shape[0], num_sample, replace=replace)
    return pc[choices], choices


def load_demo_data(points_or_path, num_point=80000, no_height=False, seed=10):
    """demo.py:24-48 without colours (use_color_* are False in ISCNet_test.yaml)."""
    import torch
    if isinstance(points_or_path, str):
        pc = read_off(points_or_path)[0]
    else:
        pc = np.asarray(points_or_path, dtype=np.float64)
    pc = pc[:, 0:3]
    if not no_height:
        floor_height = np.percentile(pc[:, 2], 0.99)           # 0.99-th percentile, as the reference
        pc = np.concatenate([pc, (pc[:, 2] - floor_height)[:, None]], 1)
    pc, _ = random_sampling(pc, num_point, np.random.default_rng(seed))
    return {'point_clouds': torch.from_numpy(pc.astype(np.float32)[None])}


def write_mesh_ply(path, vertices, faces, normals=None):
    """Binary PLY of a triangle mesh; normals (V,3): per-vertex `nx ny nz` after x y z (trimesh's vertex-normal layout).
    Without normals the file is the plain x y z one."""
    v = np.asarray(vertices, dtype=np.float32)
    f = np.asarray(faces, dtype=np.int32)
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        n = np.asarray(normals, dtype=np.float32).reshape(v.shape[0], 3)
        props += "property float nx\nproperty float ny\nproperty float nz\n"
        v = np.concatenate([v.reshape(-1, 3), n], axis=1)
    header = ("ply\nformat binary_little_endian 1.0\ncomment rfdnet_amd\nelement vertex %d\n"
              "%selement face %d\n"
              "property list uchar int vertex_indices\nend_header\n" % (v.shape[0], props, f.shape[0]))
    rec = np.empty(f.shape[0], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    rec['n'] = 3
    rec['i'] = f
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.astype('<f4').tobytes())
        fh.write(rec.tobytes())


def read_mesh_ply(path, return_normals=False):
    """-> vertices (V,3), faces (F,3) [, normals (V,3) or None when the file has none]"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in head if l.startswith("element face")][0].split()[-1])
    has_n = "property float nx" in head
    w = 6 if has_n else 3
    vn = np.frombuffer(data, dtype='<f4', count=nv * w, offset=end).reshape(nv, w)
    rec = np.frombuffer(data, dtype=[('n', 'u1'), ('i', '<i4', (3,))], count=nf, offset=end + nv * 4 * w)
    v, f = vn[:, :3].copy(), rec['i'].copy()
    if return_normals:
        return v, f, (vn[:, 3:].copy() if has_n else None)
    return v, f


_PLY_TYPES = {'char': 'i1', 'uchar': 'u1', 'short': 'i2', 'ushort': 'u2', 'int': 'i4', 'uint': 'u4', 'float': 'f4',
              'double': 'f8', 'int8': 'i1', 'uint8': 'u1', 'int16': 'i2', 'uint16': 'u2', 'int32': 'i4', 'uint32': 'u4',
              'float32': 'f4', 'float64': 'f8'}


def read_scan_ply(path):
    """-> (N,6) float32: x y z and red green blue (0 .. 255; zeros when the file has no colours) of the vertex element
    of a PLY as scanners write it (ScanNet's *_vh_clean_2.ply: float xyz, uchar rgba), ascii or binary little endian.
    The vertex element must come first and hold scalar properties only."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = [l.split() for l in data[:end].decode("ascii").split("\n") if l.strip()]
    fmt = [l[1] for l in head if l[0] == "format"][0]
    elements = [k for k, l in enumerate(head) if l[0] == "element"]
    if not elements or head[elements[0]][1] != "vertex":
        raise ValueError("%s: the vertex element must come first" % path)
    nv = int(head[elements[0]][2])
    props = [l for l in head[elements[0] + 1:(elements + [len(head)])[1]] if l[0] == "property"]
    if any(l[1] == "list" for l in props):
        raise ValueError("%s: a list property in the vertex element" % path)
    names = [l[2] for l in props]
    if fmt == "ascii":
        rows = np.array([r.split() for r in data[end:].decode("ascii").split("\n")[:nv]], dtype=np.float64)
        col = lambda name: rows[:, names.index(name)]
    elif fmt == "binary_little_endian":
        rec = np.frombuffer(data, dtype=[(l[2], '<' + _PLY_TYPES[l[1]]) for l in props], count=nv, offset=end)
        col = lambda name: rec[name]
    else:
        raise ValueError("%s: format %s is not supported" % (path, fmt))
    out = np.zeros((nv, 6), np.float32)
    for k, name in enumerate(("x", "y", "z")):
        out[:, k] = col(name)
    if all(c in names for c in ("red", "green", "blue")):
        for k, name in enumerate(("red", "green", "blue")):
            out[:, 3 + k] = col(name)
    return out


def read_mesh(path):
    """a mesh file by its extension -> (vertices (V,3) float64, faces (F,3) int32): .off (colour columns dropped,
    polygons fanned from their first corner), .obj (read_obj) or .ply (read_mesh_ply, widened); else ValueError"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".off":
        v, faces = read_off(path)
        tris = [[f[0], f[k], f[k + 1]] for f in faces for k in range(1, len(f) - 1)]
        return v[:, :3], np.asarray(tris, np.int32).reshape(-1, 3)
    if ext == ".obj":
        return read_obj(path)
    if ext == ".ply":
        v, f = read_mesh_ply(path)
        return v.astype(np.float64), f.astype(np.int32)
    raise ValueError("%s: a mesh file is .off, .obj or .ply" % path)


def write_points_ply(path, points):
    p = np.asarray(points, dtype=np.float32)[:, :3]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n"
              "property float y\nproperty float z\nend_header\n" % p.shape[0])
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(p.astype('<f4').tobytes())


def save_visualization(output_dir, point_clouds, proposal_ids, meshes, box_params=None, keep_mask=None,
                       batch_id=0):
    """Files of demo.py:278-327.  box_params (K_all,7) = centre, size, heading of
    every proposal; keep_mask (K_all,) selects the dumped ones."""
    os.makedirs(output_dir, exist_ok=True)
    ids = np.asarray(proposal_ids).reshape(-1, 1)
    for mesh, pid in zip(meshes, ids[:, 0]):
        v = mesh.vertices.cpu().numpy() if hasattr(mesh.vertices, "cpu") else mesh.vertices
        f = mesh.faces.cpu().numpy() if hasattr(mesh.faces, "cpu") else mesh.faces
        n = getattr(mesh, "vertex_normals", None)
        if n is not None and hasattr(n, "cpu"):
            n = n.cpu().numpy()
        write_mesh_ply(os.path.join(output_dir, 'proposal_%d_mesh.ply' % int(pid)), v, f, n)
    write_points_ply(os.path.join(output_dir, '%06d_pc.ply' % batch_id), np.asarray(point_clouds)[batch_id])
    if box_params is not None:
        bp = np.asarray(box_params, dtype=np.float64)
        if keep_mask is not None:
            bp = bp[np.asarray(keep_mask, dtype=bool)]
        np.savez(os.path.join(output_dir, '%06d_pred_confident_nms_bbox.npz' % batch_id),
                 obbs=bp, proposal_map=ids.astype(np.int64))


def write_png(path, image):
    """image (H,W,3) uint8 -> an 8-bit RGB PNG without interlace (filter 0 on every row)"""
    img = np.ascontiguousarray(np.asarray(image))
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("write_png: an (H,W,3) uint8 image, got %s %s" % (img.dtype, img.shape))
    h, w = img.shape[:2]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * 3)], 1)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                 chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def save_scene(output_dir, scene_mesh, render=None):
    """scene_objects.ply: the placed objects of iscnet.scene.place_objects as one mesh (with nx ny nz if it has normals);
    pred.png: render.image of rfdnet_amd.render.render_scene, if given"""
    os.makedirs(output_dir, exist_ok=True)
    host = lambda t: None if t is None else t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    write_mesh_ply(os.path.join(output_dir, 'scene_objects.ply'), host(scene_mesh.vertices), host(scene_mesh.faces),
                   host(scene_mesh.normals))
    if render is not None:
        write_png(os.path.join(output_dir, 'pred.png'), host(render.image))

"""The rules of include/rfd_fuse.h in numpy float32 (no test in here): `fuse` is the reference's CPU fusion (external/pyfusion
fusion.cpp + fusion.h: fusion_tsdf_cpu, and fusion_tsdfmask_cpu as count > 0), operation for operation, so its bits are the
reference's (tests/test_fuse_cpu.py holds it to tests/golden/F_FUSE.npz); `depth_from_keys` is rule 6."""
import numpy as np

F = np.float32


def voxel_centres(n, vx_size):
    """rule 1: (float)((i + 0.5) * (double)vx_size - 0.5) for i < n"""
    return ((np.arange(n, dtype=np.float64) + 0.5) * np.float64(F(vx_size)) - 0.5).astype(F)


def fuse(depth, K, R, T, shape, vx_size, truncation, unknown_is_free, unobserved_value):
    """depth (V,rows,cols), K (V,9) or (V,3,3), R likewise, T (V,3), shape (D,H,W) -> tsdf (D,H,W) f32, count (D,H,W) i32"""
    D, H, W = (int(s) for s in shape)
    depth = np.asarray(depth, F)
    V = depth.shape[0]
    rows, cols = depth.shape[1:] if depth.ndim == 3 else (1, 1)
    K, R, T = (np.asarray(a, F).reshape(V, n) for a, n in ((K, 9), (R, 9), (T, 3)))
    t, unobserved_value = F(truncation), F(unobserved_value)
    z, y, x = np.meshgrid(voxel_centres(D, vx_size), voxel_centres(H, vx_size), voxel_centres(W, vx_size), indexing='ij')
    total, count = np.zeros((D, H, W), F), np.zeros((D, H, W), np.int32)
    with np.errstate(all='ignore'):
        for v in range(V):
            k, r, o = K[v], R[v], T[v]
            xt = ((r[0] * x + r[1] * y) + r[2] * z) + o[0]                    # f32 throughout: every operand is f32
            yt = ((r[3] * x + r[4] * y) + r[5] * z) + o[1]
            zt = ((r[6] * x + r[7] * y) + r[8] * z) + o[2]
            u = (k[0] * xt + k[1] * yt) + k[2] * zt
            w = (k[3] * xt + k[4] * yt) + k[5] * zt
            dd = (k[6] * xt + k[7] * yt) + k[8] * zt
            tu, tv = u / dd + F(0.5), w / dd + F(0.5)
            on = (tu > F(-1)) & (tu < F(cols)) & (tv > F(-1)) & (tv < F(rows))      # rule 3: false for a NaN
            pu, pv = np.where(on, tu, F(0)).astype(np.int64), np.where(on, tv, F(0)).astype(np.int64)
            g = depth[v][pv, pu]
            if unknown_is_free:
                g = np.where(g < 0, F(1e9), g)
            dist = g - dd
            valid = on & (g > 0) & (dist >= -t)
            total = np.where(valid, total + np.minimum(t, np.maximum(-t, dist)), total)
            count = count + valid.astype(np.int32)
        assert total.dtype == F
        tsdf = np.where(count > 0, total / np.maximum(count, 1).astype(F), unobserved_value).astype(F)
    return tsdf, count


def key_depth(keys, far):
    """keys (H,W) u64 -> z (H,W) f32: far where the key is 0 or z > far, else (float)(1 / (double)invz)"""
    keys = np.asarray(keys).astype(np.uint64)
    invz = (keys >> np.uint64(32)).astype(np.uint32).view(F)
    with np.errstate(all='ignore'):
        z = (1.0 / invz.astype(np.float64)).astype(F)
    far = F(far)
    return np.where((keys == 0) | (z > far), far, z).astype(F)


def erode3(a):
    """the minimum over the 3x3 neighbourhood cut at the border (scipy.ndimage.grey_erosion(size=(3,3)), `reflect`)"""
    p = np.pad(a, 1, mode='edge')
    H, W = a.shape
    return np.min(np.stack([p[j:j + H, i:i + W] for j in range(3) for i in range(3)]), 0)


def depth_from_keys(keys, far, offset):
    """rule 6"""
    return erode3(key_depth(keys, far) - F(offset))

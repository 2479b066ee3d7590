"""CPU restatement of vgx_submaps_generate_separated_mesh (include/voxgraph_amd.h): cblox SubmapMesher::
generateSeparatedMesh.  Each submap is meshed in its own frame by tests/mesh_ref.py (the restatement of
vgx_submap_generate_mesh), its vertices moved by the f32 transform of tests/projected_map_ref.py and its normals turned
by the same rotation (not renormalised), every triangle coloured with the submap's colour; then the per-block meshes are
combined by submap-frame block index, ascending, the submaps' triangles in array order within a block.

Also voxblox's rainbowColorMap [recalled], written out case by case."""
import math

import numpy as np

from tests import mesh_ref as mr
from tests import projected_map_ref as pm

F = np.float32


def rainbow_color_map(h):
    """voxblox rainbowColorMap(h): HSV blend at s = v = 1 in double, channels truncated to uint8, a = 255"""
    h = float(h)
    h = h - math.floor(h)
    h = h * 6.0
    i = int(math.floor(h))
    f = h - i
    if i % 2 == 0:
        f = 1.0 - f
    n = 1.0 - f
    if i in (0, 6):
        r, g, b = 255.0, 255.0 * n, 0.0
    elif i == 1:
        r, g, b = 255.0 * n, 255.0, 0.0
    elif i == 2:
        r, g, b = 0.0, 255.0, 255.0 * n
    elif i == 3:
        r, g, b = 0.0, 255.0 * n, 255.0
    elif i == 4:
        r, g, b = 255.0 * n, 0.0, 255.0
    elif i == 5:
        r, g, b = 255.0, 0.0, 255.0 * n
    else:
        r, g, b = 255.0, 127.0, 127.0
    return np.array([int(r), int(g), int(b), 255], np.uint8)


def submap_color(submap_id, cycle=20):
    return rainbow_color_map(float(submap_id) / float(cycle))


def pose_mesh(mesh, T):
    """(block_index, first, vertices, normals) in the submap frame -> the same at pose T [7] (qw,qx,qy,qz, tx,ty,tz)"""
    bi, first, v, n = mesh[:4]
    T = np.asarray(T, F)
    q, t = T[:4], T[4:7]
    v2 = pm.transform(q, t, v.reshape(-1, 3)).reshape(v.shape).astype(F)
    n2 = pm.quat_rotate(q, n.reshape(-1, 3)).reshape(n.shape).astype(F)
    return bi, first, v2, n2


def combine(meshes, colors):
    """meshes: per submap (block_index [nb][3], first [nb+1], vertices, normals), already posed; colors [n][4] uint8.
    Returns (block_index [nb][3] int32, first [nb+1] int64, vertices [T][3][3] f32, normals [T][3] f32, rgba [T][4] u8)."""
    entries = {}
    for s, (bi, first, v, n) in enumerate(meshes):
        for k, b in enumerate(np.asarray(bi, np.int64).reshape(-1, 3)):
            entries.setdefault(tuple(int(c) for c in b), []).append((s, int(first[k]), int(first[k + 1])))
    keys = sorted(entries)
    out_bi = np.array(keys, np.int32).reshape(-1, 3)
    first = np.zeros(len(keys) + 1, np.int64)
    vs, ns, cs = [np.zeros((0, 3, 3), F)], [np.zeros((0, 3), F)], [np.zeros((0, 4), np.uint8)]
    for j, key in enumerate(keys):
        tot = 0
        for s, a, b in entries[key]:                     # (array order: appended in s order)
            vs.append(meshes[s][2][a:b])
            ns.append(meshes[s][3][a:b])
            cs.append(np.repeat(np.asarray(colors[s], np.uint8).reshape(1, 4), b - a, 0))
            tot += b - a
        first[j + 1] = first[j] + tot
    return out_bi, first, np.concatenate(vs).astype(F), np.concatenate(ns).astype(F), np.concatenate(cs)


def separated_mesh(subs, poses, colors, vps, voxel_size, min_weight=1e-4):
    """subs: per submap (block_index [n][3], distance [n][vps^3], weight [n][vps^3]) in the submap frame; poses [n][7];
    colors [n][4].  The submaps in ARRAY order.  Returns combine()'s tuple."""
    meshes = [pose_mesh(mr.generate_mesh(bi, d, w, vps, voxel_size, min_weight), T) for (bi, d, w), T in zip(subs, poses)]
    return combine(meshes, colors)

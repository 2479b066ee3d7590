"""The combined mesh without a GPU: the marching-cubes triangle table the kernels use (read through the library)
checked row by row for its topology, the vectorised restatement (tests/mesh_ref.py) against a literal per-cube
transcription of voxblox's loops, and analytic spheres meshed by the restatement checked for closure, genus, normals
and area."""
import numpy as np
import pytest

from tests import mesh_ref as mr

F = np.float32
# the cube faces as sets of their four edges
FACES = [{0, 1, 2, 3}, {4, 5, 6, 7}, {0, 4, 8, 9}, {2, 6, 10, 11}, {3, 7, 8, 11}, {1, 5, 9, 10}]


def _rows():
    t = mr.triangle_table()
    out = []
    for c in range(256):
        r = [int(v) for v in t[c]]
        n = r.index(-1) if -1 in r else 16
        assert n % 3 == 0 and all(v == -1 for v in r[n:]), c
        out.append([tuple(r[3 * k:3 * k + 3]) for k in range(n // 3)])
    return out


def _crossing(c):
    return {e for e, (a, b) in enumerate(mr.EDGES) if ((c >> a) & 1) != ((c >> b) & 1)}


def test_table_shape_and_empty_rows():
    rows = _rows()
    assert rows[0] == [] and rows[255] == []
    assert max(len(r) for r in rows) == 5
    assert all(len(r) > 0 for r in rows[1:255])
    assert all(0 <= e < 12 for r in rows for t in r for e in t)


def test_table_uses_exactly_the_sign_changing_edges():
    for c, tris in enumerate(_rows()):
        assert {e for t in tris for e in t} == _crossing(c), c


def test_table_interior_sides_shared_twice_with_opposite_orientation():
    for c, tris in enumerate(_rows()):
        sides = {}
        for t in tris:
            assert len(set(t)) == 3, (c, t)
            for i in range(3):
                a, b = t[i], t[(i + 1) % 3]
                sides.setdefault(frozenset((a, b)), []).append((a, b))
        for s, uses in sides.items():
            if any(s <= f for f in FACES):
                assert len(uses) == 1, (c, sorted(s), uses)            # a face segment: the patch's boundary
            else:
                assert len(uses) == 2 and uses[0] == uses[1][::-1], (c, sorted(s), uses)


def test_table_face_segments_join_the_face_crossings():
    ambiguous = 0
    for c, tris in enumerate(_rows()):
        segs = {frozenset((t[i], t[(i + 1) % 3])) for t in tris for i in range(3)}
        for f in FACES:
            on = [s for s in segs if s <= f]
            cross = _crossing(c) & f
            assert sorted(e for s in on for e in s) == sorted(cross), (c, sorted(f), on)
            if len(cross) == 2:
                assert on == [frozenset(cross)], (c, sorted(f))        # the only possible pairing
            elif len(cross) == 4:
                ambiguous += 1
                for s in on:                                           # two segments, each cutting off one corner
                    a, b = tuple(s)
                    assert set(mr.EDGES[a]) & set(mr.EDGES[b]), (c, sorted(f), on)
    assert ambiguous > 0


def test_table_orientation_points_to_positive_side():
    # emitted order e2, e1, e0 at the edge midpoints: the normal leans from the negative corners to the positive ones
    P = mr.CORNERS.astype(float)
    for c, tris in enumerate(_rows()):
        for t in tris:
            p = [0.5 * (P[mr.EDGES[e][0]] + P[mr.EDGES[e][1]]) for e in t[::-1]]
            n = np.cross(p[1] - p[0], p[2] - p[0])
            lean = 0.0
            for e in t:
                a, b = mr.EDGES[e]
                neg, pos = (a, b) if (c >> a) & 1 else (b, a)
                lean += float(n @ (P[pos] - P[neg]))
            assert lean > 0, (c, t)


# ---- the restatement against a literal transcription ------------------------------------------------------------------

def literal_mesh(block_index, distance, weight, vps, voxel_size, min_weight):
    """MeshIntegrator::generateMesh(false, false) [recalled], one cube at a time in f32 scalars"""
    vs, mw = F(voxel_size), F(min_weight)
    table = mr.triangle_table()
    blocks = {tuple(int(c) for c in b): i for i, b in enumerate(np.asarray(block_index).reshape(-1, 3))}
    bs = F(F(vps) * vs)

    def corner(b, x, y, z):
        gb = (b[0] + x // vps, b[1] + y // vps, b[2] + z // vps)
        i = blocks.get(gb)
        if i is None:
            return None
        lin = (x % vps) + vps * ((y % vps) + vps * (z % vps))
        if not weight[i][lin] > mw:                                     # getSdfIfValid
            return None
        return distance[i][lin]

    out_bi, first, verts, norms = [], [0], [], []
    for b in sorted(blocks):
        order = [(x, y, z) for x in range(vps - 1) for y in range(vps - 1) for z in range(vps - 1)]
        order += [(vps - 1, y, z) for z in range(vps) for y in range(vps)]
        order += [(x, vps - 1, z) for z in range(vps) for x in range(vps - 1)]
        order += [(x, y, vps - 1) for y in range(vps - 1) for x in range(vps - 1)]
        for x, y, z in order:
            sdf = [corner(b, x + o[0], y + o[1], z + o[2]) for o in mr.CORNERS]
            if any(s is None for s in sdf):
                continue
            coords = [F(F(b[a]) * bs) + F((F(v) + F(0.5)) * vs) for a, v in enumerate((x, y, z))]
            pts = [[F(coords[a] + (vs if o[a] else F(0))) for a in range(3)] for o in mr.CORNERS]
            cfg = sum(1 << i for i in range(8) if sdf[i] < 0)
            k = 0
            while table[cfg][k] != -1:
                tri = []
                for e in (table[cfg][k + 2], table[cfg][k + 1], table[cfg][k]):
                    a, c = mr.EDGES[e]
                    sa, sb = F(sdf[a]), F(sdf[c])
                    diff = F(sa - sb)
                    if abs(diff) >= F(1e-6):
                        t = F(sa / diff)
                        tri.append([F(pts[a][q] + F(t * F(pts[c][q] - pts[a][q]))) for q in range(3)])
                    else:
                        tri.append([F(F(0.5) * F(pts[a][q] + pts[c][q])) for q in range(3)])
                u = [F(tri[1][q] - tri[0][q]) for q in range(3)]
                v = [F(tri[2][q] - tri[0][q]) for q in range(3)]
                n = [F(u[1] * v[2] - u[2] * v[1]), F(u[2] * v[0] - u[0] * v[2]), F(u[0] * v[1] - u[1] * v[0])]
                sq = F(F(F(n[0] * n[0]) + F(n[1] * n[1])) + F(n[2] * n[2]))
                if sq > 0:
                    ln = F(np.sqrt(sq))
                    n = [F(c / ln) for c in n]
                verts.append(tri)
                norms.append(n)
                k += 3
        out_bi.append(b)
        first.append(len(verts))
    return (np.array(out_bi, np.int32).reshape(-1, 3), np.array(first, np.int64), np.array(verts, F).reshape(-1, 3, 3),
            np.array(norms, F).reshape(-1, 3))


def edge_case_layer(rng, vps, block_min, block_dims, density=0.8, min_weight=1e-4):
    """random sdf around 0 with the corner cases of section 1 planted: missing neighbours, weight == min_weight,
    sdf == 0 corners, |sa - sb| < 1e-6 pairs, negative block indices"""
    g = np.stack(np.meshgrid(*[np.arange(m, m + d) for m, d in zip(block_min, block_dims)], indexing="ij"), -1).reshape(-1, 3)
    bi = g[rng.random(len(g)) < density].astype(np.int32)
    n, nv = len(bi), vps ** 3
    d = rng.uniform(-0.3, 0.3, (n, nv)).astype(F)
    w = rng.uniform(0.5, 5, (n, nv)).astype(F)
    w[rng.random(w.shape) < 0.03] = 0
    w[rng.random(w.shape) < 0.03] = F(min_weight)                       # not valid: weight must exceed min_weight
    d[rng.random(d.shape) < 0.05] = 0                                   # zero corners: degenerate triangles
    tiny = rng.random(d.shape) < 0.05
    d[tiny] = rng.uniform(-4e-7, 4e-7, tiny.sum()).astype(F)            # near-equal pairs of opposite sign
    d[rng.random(d.shape) < 0.02] = F(-0.0)
    return bi, d, w


def _assert_same(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape, (x.shape, y.shape)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.parametrize("vps,seed", [(4, 0), (4, 1), (8, 2)])
def test_restatement_equals_literal_transcription(vps, seed):
    rng = np.random.default_rng(seed)
    dims = (3, 3, 2) if vps == 4 else (2, 2, 2)
    bi, d, w = edge_case_layer(rng, vps, (-2, -1, -1), dims)
    perm = rng.permutation(len(bi))                                     # input order must not matter
    got = mr.generate_mesh(bi[perm], d[perm], w[perm], vps, 0.1, 1e-4)
    want = literal_mesh(bi, d, w, vps, 0.1, 1e-4)
    _assert_same(got[:4], want)
    assert len(want[2]) > 100
    n = got[3]
    assert (np.abs(n).sum(1) == 0).any()                                # a degenerate triangle kept its zero normal


def test_restatement_small_cases():
    vps = 4
    empty = mr.generate_mesh(np.zeros((0, 3), np.int32), np.zeros((0, 64), F), np.zeros((0, 64), F), vps, 0.1)
    assert empty[0].shape == (0, 3) and list(empty[1]) == [0] and len(empty[2]) == 0
    # a lone block: only its interior cubes are meshed (every cube touching the max planes lacks a neighbour)
    rng = np.random.default_rng(5)
    d = rng.uniform(-1, 1, (1, 64)).astype(F)
    w = np.ones((1, 64), F)
    bi, first, v, n, k = mr.generate_mesh(np.array([[-3, 2, -1]]), d, w, vps, 0.1)
    assert first[-1] == len(v) and (k[..., :3] // vps <= np.array([-3, 2, -1])).all()
    assert np.array_equal(literal_mesh(np.array([[-3, 2, -1]]), d, w, vps, 0.1, 1e-4)[2].view(np.uint32), v.view(np.uint32))


# ---- analytic spheres -------------------------------------------------------------------------------------------------

def sphere_layer(centre, radius, vps, vs):
    """sdf = |p - c| - r at every voxel centre of a dense block box around the sphere, weight 1"""
    bs = vps * vs
    lo = np.floor((np.asarray(centre) - radius - 2 * vs) / bs).astype(int) - 1
    hi = np.floor((np.asarray(centre) + radius + 2 * vs) / bs).astype(int) + 1
    g = np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(lo, hi)], indexing="ij"), -1).reshape(-1, 3)
    i = np.arange(vps ** 3)
    local = (np.stack([i % vps, (i // vps) % vps, i // (vps * vps)], -1) + 0.5) * vs
    p = g[:, None, :] * bs + local[None]
    d = (np.linalg.norm(p - np.asarray(centre), axis=-1) - radius).astype(F)
    return g.astype(np.int32), d, np.ones_like(d)


def check_sphere(mesh, centre, radius):
    _, first, v, n, keys = mesh
    T = len(v)
    assert T > 100
    # closed, keyed by grid edge: every side in exactly two triangles, in opposite directions
    kid = {}
    ids = np.array([[kid.setdefault(tuple(k), len(kid)) for k in tri] for tri in keys.reshape(-1, 3, 4)])
    directed = {}
    for t in ids:
        for i in range(3):
            s = (t[i], t[(i + 1) % 3])
            assert s not in directed, s
            directed[s] = 1
    assert all((b, a) in directed for a, b in directed)
    n_edges = len(directed) // 2
    assert len(kid) - n_edges + T == 2                                   # Euler characteristic of a sphere
    # normals point towards positive distance (outwards)
    centroid = v.astype(np.float64).mean(1)
    good = np.abs(n).sum(1) > 0
    assert (np.einsum("ij,ij->i", n[good], centroid[good] - centre) > 0).all()
    area = 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1).sum()
    assert abs(area / (4 * np.pi * radius ** 2) - 1) < 0.02, area / (4 * np.pi * radius ** 2)


@pytest.mark.parametrize("radius_vox,seed", [(6, 0), (9.5, 1), (14, 2)])
def test_sphere_restatement(radius_vox, seed):
    rng = np.random.default_rng(seed)
    vps, vs = 8, 0.1
    centre = rng.uniform(-0.5, 0.5, 3)
    bi, d, w = sphere_layer(centre, radius_vox * vs, vps, vs)
    check_sphere(mr.generate_mesh(bi, d, w, vps, vs), centre, radius_vox * vs)

"""Triangle mesh -> exact signed distance, the parts that need no GPU: sdfhip_trimesh_prepare against known pseudonormals and against
the restatement's own preparation, its refusals, the fit; the restatement (tests/trimesh_restatement.py) against closed-form truth
it did not make -- the box distance and the sphere -- on its float distances before quantisation; the readers of files with faces;
the pruned restatement against the brute-force one on the adversarial soups, and those soups' ties and NaN."""
import ctypes
import os
import struct

import numpy as np
import pytest

import mesh_restatement as mr
import trimesh_restatement as tr

f32 = np.float32
EPS = float(np.finfo(f32).eps)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


_cache = {}


def sphere_mesh(sb):
    if "sphere" not in _cache:
        od = sb.sphere_d4()
        _cache["sphere"] = mr.mesh(od.Structs, od.Values, -1)[..., :3].copy()
    return _cache["sphere"]


def test_prepare_cube_pseudonormals(sb):
    soup = tr.cube()
    with sb.TriMesh.FromSoup(soup) as m:
        R = m.records.copy()
        assert (m.n_vertices, m.n_edges, m.n_records, m.n_dropped, m.open_edges) == (8, 18, 12, 0, 0)
        assert m.n_vertices - m.n_edges + m.n_records == 2
        assert m.scale == 1.0 and m.offset == (0.0, 0.0, 0.0)
    assert same_bits(R[:, :9], soup.reshape(-1, 9)) and (R[:, 30].view(np.uint32) == np.arange(12)).all() and (R[:, 31] == 0).all()
    # the corners meet 3, 4, 5 and 6 triangles
    corners, count = np.unique(soup.reshape(-1, 3), axis=0, return_counts=True)
    assert sorted(set(count.tolist())) == [3, 4, 5, 6]
    # angle weighting: every vertex pseudonormal is the corner's diagonal, however the faces were cut
    for k in range(3):
        pos, n = R[:, 3 * k:3 * k + 3].astype(np.float64), R[:, 21 + 3 * k:24 + 3 * k].astype(np.float64)
        want = np.sign(pos - 0.5) / np.sqrt(3.0)
        assert np.abs(n - want).max() <= 4 * EPS
    # area or uniform weighting would not give that on this cube (the test would pass with a wrong rule otherwise)
    face = R[:, 9:12].astype(np.float64)
    for corner in corners[count != 3][:1]:
        at = (soup.reshape(-1, 3, 3) == corner).all(2).any(1)
        uniform = face[at].sum(0) / np.linalg.norm(face[at].sum(0))
        assert np.abs(uniform - np.sign(corner - 0.5) / np.sqrt(3.0)).max() > 1e-3
    # edge pseudonormals: the normalised sum of the two faces on the edge
    tri = soup.astype(np.float64)
    for t in range(12):
        for k in range(3):
            a, b = tri[t, k], tri[t, (k + 1) % 3]
            on = [u for u in range(12) if (tri[u] == a).all(1).any() and (tri[u] == b).all(1).any()]
            assert len(on) == 2
            s = face[on[0]] + face[on[1]]
            assert np.abs(R[t, 12 + 3 * k:15 + 3 * k] - s / np.linalg.norm(s)).max() <= 4 * EPS


@pytest.mark.parametrize("name", ["cube", "tetrahedron", "l_prism", "sphere"])
def test_prepare_is_the_restatements(sb, name):
    soup = sphere_mesh(sb) if name == "sphere" else getattr(tr, name)()
    want, counts = tr.prepare(soup)
    with sb.TriMesh.FromSoup(soup) as m:
        got = m.records.copy()
        assert dict(n_vertices=m.n_vertices, n_edges=m.n_edges, n_records=m.n_records, n_dropped=m.n_dropped, open_edges=m.open_edges) == counts
    assert same_bits(got[:, :9], want[:, :9]) and same_bits(got[:, 30:], want[:, 30:])
    assert np.abs(got[:, 9:30].astype(np.float64) - want[:, 9:30]).max() <= 4 * EPS
    if name == "sphere":
        assert counts["n_records"] == 2520 and counts["open_edges"] == 0 and counts["n_dropped"] == 0
    if name == "l_prism":
        assert (counts["n_vertices"], counts["n_edges"], counts["n_records"], counts["open_edges"]) == (12, 30, 20, 0)
    # stride 6 (sdfhip_mesh.verts6) gives the same records, whatever the normals say
    six = np.concatenate([soup, np.full_like(soup, np.nan)], axis=2)
    with sb.TriMesh.FromMesh(six) as m:
        assert same_bits(m.records, got)


def test_prepare_bad_input(sb):
    L = sb._lib
    soup = tr.cube()
    with sb.TriMesh.FromSoup(soup[:10]) as m:                   # two triangles removed
        assert m.open_edges == 4 and m.n_records == 10
    flat = np.array([[[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3]]], dtype=f32)       # zero area
    with sb.TriMesh.FromSoup(np.concatenate([soup[:5], flat, soup[5:]])) as m:
        assert (m.n_dropped, m.n_records, m.open_edges) == (1, 12, 0)
        assert (m.records[:, 30].view(np.uint32) == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12]).all()
        want = tr.prepare(np.concatenate([soup[:5], flat, soup[5:]]))[0]
        assert same_bits(m.records[:, 30], want[:, 30])
    bad = soup.copy()
    bad[3, 1, 2] = np.nan
    for what in (bad, flat, np.concatenate([flat, flat]), soup * f32(3000.0)):
        with pytest.raises(sb.SdfHipError) as e:
            sb.TriMesh.FromSoup(what)
        assert e.value.code == L.ERR_ARG
    raw = L.CTriMesh()
    assert L.lib.sdfhip_trimesh_prepare(soup.ctypes.data, 0, 3, None, ctypes.byref(raw)) == L.ERR_ARG       # n = 0
    assert L.lib.sdfhip_trimesh_prepare(soup.ctypes.data, 12, 4, None, ctypes.byref(raw)) == L.ERR_ARG      # stride
    assert L.lib.sdfhip_trimesh_prepare(None, 12, 3, None, ctypes.byref(raw)) == L.ERR_ARG
    assert L.lib.sdfhip_trimesh_prepare(soup.ctypes.data, 12, 3, None, None) == L.ERR_ARG
    # the options' size rules are sdfhip_mesh_options': too small, not a multiple of 4, unknown fields set
    opt = L.TriMeshOptions()
    L.lib.sdfhip_trimesh_options_default(ctypes.byref(opt))
    assert (opt.size, opt.fit, opt.fill) == (12, -1, -1.0)
    assert L.lib.sdfhip_trimesh_prepare(soup.ctypes.data, 12, 3, ctypes.byref(opt), ctypes.byref(raw)) == L.OK
    L.lib.sdfhip_trimesh_free(ctypes.byref(raw))
    assert not raw.records and raw.n_records == 0
    for size in (8, 0, 14, 8192):
        opt.size = size
        assert L.lib.sdfhip_trimesh_prepare(soup.ctypes.data, 12, 3, ctypes.byref(opt), ctypes.byref(raw)) == L.ERR_ARG, size

    class Grown(ctypes.Structure):
        _fields_ = [("base", L.TriMeshOptions), ("more", ctypes.c_int32)]
    for more, rc in ((-1, L.OK), (0, L.ERR_ARG)):
        g = Grown(L.TriMeshOptions(), more)
        g.base.size = ctypes.sizeof(Grown)
        assert L.lib.sdfhip_trimesh_prepare(soup.ctypes.data, 12, 3, ctypes.cast(ctypes.byref(g), ctypes.POINTER(L.TriMeshOptions)), ctypes.byref(raw)) == rc
        L.lib.sdfhip_trimesh_free(ctypes.byref(raw))
    for fit, fill in ((2, None), (1, 0.0), (1, float("nan")), (1, 2000.0)):
        with pytest.raises(sb.SdfHipError):
            sb.TriMesh.FromSoup(soup, fit=fit, fill=fill)


def test_fit_maps_the_bounding_box_as_pinned(sb):
    soup = (tr.l_prism() * f32(37.5) - f32(11.0)) * np.array([1.0, 0.6, 0.3], dtype=f32)
    for fill in (None, 0.5):
        want_pos, s, mid = tr.fit_positions(soup, 0.8 if fill is None else fill)
        with sb.TriMesh.FromSoup(soup, fit=1, fill=fill) as m:
            assert same_bits(m.records[:, :9], (want_pos + f32(0)).reshape(-1, 9))
            assert same_bits([m.scale], [s]) and same_bits(m.offset, mid)
            lo, hi = m.records[:, :9].reshape(-1, 3).min(0), m.records[:, :9].reshape(-1, 3).max(0)
            assert abs(float((hi - lo).max()) - (0.8 if fill is None else fill)) < 1e-6 and np.abs((lo + hi) / 2 - 0.5).max() < 1e-6
            want = tr.prepare(soup, fit=1, fill=0.8 if fill is None else fill)[0]
            assert same_bits(m.records[:, :9], want[:, :9]) and np.abs(m.records[:, 9:30].astype(np.float64) - want[:, 9:30]).max() <= 4 * EPS


def box_distance(p, lo=0.25, hi=0.75):
    """closed form, double: the signed distance to the box [lo, hi]^3"""
    p = np.asarray(p, dtype=np.float64)
    q = np.abs(p - (lo + hi) / 2) - (hi - lo) / 2
    return np.sqrt((np.maximum(q, 0) ** 2).sum(1)) + np.minimum(q.max(1), 0)


def test_restatement_against_the_closed_form_box():
    R = tr.prepare(tr.cube())[0]
    rng = np.random.default_rng(2024)
    p = rng.uniform(0.0, 1.0, (20_000, 3)).astype(f32)
    q = np.abs(p.astype(np.float64) - 0.5) - 0.25
    outside_axes = (q > 0).sum(1)
    assert all((outside_axes == k).sum() > 100 for k in (0, 1, 2, 3))        # inside, nearest a face, an edge, a corner
    got = tr.values(R, p).astype(np.float64)
    assert np.abs(got - box_distance(p)).max() <= 2.0 ** -20


def test_restatement_against_the_sphere(sb):
    soup = sphere_mesh(sb)
    R, counts = tr.prepare(soup)
    assert counts["n_records"] == 2520 and counts["open_edges"] == 0
    V = soup.reshape(-1, 3).astype(np.float64)
    delta = np.abs(np.sqrt(((V - 0.5) ** 2).sum(1)) - 0.3).max()
    T = soup.astype(np.float64)
    L = max(np.sqrt(((T[:, k] - T[:, (k + 1) % 3]) ** 2).sum(1)).max() for k in range(3))
    eps = delta + L * L / (8 * (0.3 - delta))
    assert eps < 0.3 / 4                                       # (far below the radius: the bound and the sign check say something)
    _, _, floats = tr.build(R, 4, want_float=True)
    _cache["sphere_build"] = floats
    n = 0
    for depth, (coords, cv, mv) in enumerate(floats):
        S = 2.0 ** -depth
        pts = np.concatenate([((coords[:, None, :] + tr.CORNER[None]) * S).reshape(-1, 3), (coords + 0.5) * S])
        got = np.concatenate([cv.reshape(-1), mv]).astype(np.float64)
        want = np.sqrt(((pts - 0.5) ** 2).sum(1)) - 0.3
        assert np.abs(got - want).max() <= eps + 2.0 ** -20, depth
        far = np.abs(want) > eps
        assert (np.sign(got[far]) == np.sign(want[far])).all(), depth
        n += len(got)
    assert len(floats) == 5 and n > 5000


def truncated(tree, depth):
    """the depth-`depth` tree out of a deeper one: the same nodes down to that level, whose nodes are leaves"""
    structs, values, floats = tree
    n = sum(len(f[0]) for f in floats[:depth + 1])
    last = n - len(floats[min(depth, len(floats) - 1)][0])
    S = structs[:n].copy()
    if depth < len(floats) - 1:
        S[last:, 1] = -1
    return S, values[:n]


@pytest.mark.parametrize("name", list(tr.ADVERSARIAL))
def test_pruned_restatement_is_the_brute_force_one(name):
    """build_pruned (the GPU's candidate lists and their threshold, np.float32) against build (every record at every point) on the
    adversarial soups, byte for byte, depths 4 and 5 (two_sheets, 2176 records: depth 4); the lists save work"""
    R = tr.prepare(getattr(tr, name)(), fit=tr.ADVERSARIAL[name])[0]
    deepest = 4 if name == "two_sheets" else 5
    brute = tr.build(R, deepest, want_float=True)
    for depth in range(4, deepest + 1):
        S, V = truncated(brute, depth)
        gS, gV, entries = tr.build_pruned(R, depth)
        assert gS.shape == S.shape and (gS == S).all() and (gV == V).all(), depth
        blocks = 1 + int((S[:, 1] >= 0).sum())
        if len(S) > 1:
            assert len(R) < entries < blocks * len(R), (depth, entries, blocks)
        else:
            assert entries == len(R) and (V == 255).all()     # far_away: the root alone, saturated
    assert (len(S) == 1) == (name == "far_away")
    if name == "strips_far":
        assert np.abs(R[:, :9]).max() > 900
    _cache["brute", name] = (R, brute)


def test_two_sheets_tie_with_opposite_signs():
    """every lattice point on z = 0.5 over the sheets has bit-equal D to a record of sheet B and to its mirror image in sheet A,
    1088 records on, and the value carries the sign of the lower index (below B: negative)"""
    R, brute = _cache.get(("brute", "two_sheets")) or (tr.prepare(tr.two_sheets())[0], None)
    m = len(R) // 2
    assert m == 1088 and (R[:m, 2] == 0.625).all() and (R[m:, 2] == 0.375).all()
    x, y = np.meshgrid(0.375 + np.arange(9) / 32.0, 0.4375 + np.arange(5) / 32.0)      # the depth-5 lattice over the sheets
    p = np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.5)], 1).astype(f32)
    D, r, region = tr.dist2(R, p)
    assert not np.isnan(D).any()
    lower_wave = 0
    for k in range(len(p)):
        tie = np.nonzero(D[k] == D[k].min())[0]
        first = tie[0]
        assert first < m and first + m in tie and D[k, first] == f32(0.125) ** 2
        sign = lambda t: tr._dot([r[a][k, t] for a in range(3)], [R[t, tr.REGION_NORMAL[int(region[k, t])] + a] for a in range(3)])
        assert sign(first) < 0 < sign(first + m)
        for t in tie[tie < m]:                                 # a record and its image: another chunk of 1024, another wave of 64
            assert t // 1024 != (t + m) // 1024 and t % 1024 // 64 != (t + m) % 1024 // 64 and t % 256 // 64 != (t + m) % 256 // 64
        lower_wave += int((first + m) % 1024 // 64 < first % 1024 // 64)
    assert lower_wave > 0                                      # (the image sits in a lower wave: "the lowest wave wins" is wrong here)
    assert (tr.values(R, p) == f32(-0.125)).all()
    assert (tr.from_float(f32(-0.125), f32(2.0 ** -5)) != tr.from_float(f32(0.125), f32(2.0 ** -5)))


def test_sliver_has_nan_distances_in_the_tree(sb):
    """the extra triangle of `sliver` is kept by prepare and its D is NaN at corners of the depth-4 tree; a NaN never wins"""
    R, brute = _cache.get(("brute", "sliver")) or (None, None)
    if R is None:
        R = tr.prepare(tr.sliver())[0]
        brute = tr.build(R, 5, want_float=True)
    assert len(R) == 13 and R[12, 30].view(np.uint32) == 12
    coords, cv, _ = brute[2][4]
    corners = (coords[:, None, :] + tr.CORNER[None]).reshape(-1, 3).astype(f32) * f32(2.0 ** -4)
    D = tr.dist2(R[12:], corners)[0][:, 0]
    bad = np.isnan(D)
    assert bad.sum() >= 8 and (corners[bad, 0] == 0).all() and (corners[bad, 1] > 0).all()
    assert np.isfinite(cv.reshape(-1)[bad]).all()              # the cube answers there
    with sb.TriMesh.FromSoup(tr.sliver()) as m:                # the library's prepare keeps it too
        assert (m.n_dropped, m.n_records) == (0, 13) and same_bits(m.records[:, :9], R[:, :9])


def test_readers_give_back_what_the_writers_wrote(sb, tmp_path):
    rng = np.random.default_rng(3)
    tris = rng.uniform(-2, 2, (40, 3, 6)).astype(f32)
    tris[0, 0, 0] = -0.0
    tris[1, 1, 1] = np.float32(1e-41)                         # a denormal
    tris[2, 2, 2] = np.float32(-3e-45)
    tris[3, 0, 3:] = np.nan                                    # a NaN normal
    tris[4, 1, 4] = -0.0
    sb.SaveMeshPly(str(tmp_path / "m.ply"), tris)
    sb.SaveMeshObj(str(tmp_path / "m.obj"), tris)
    for got in (sb.LoadMeshPly(tmp_path / "m.ply"), sb.LoadMeshObj(tmp_path / "m.obj")):
        assert got.shape == tris.shape
        assert ((got.view(np.uint32) == tris.view(np.uint32)) | (np.isnan(got) & np.isnan(tris))).all()
    with sb.TriMesh.LoadPly(tmp_path / "m.ply") as a, sb.TriMesh.LoadObj(tmp_path / "m.obj") as b, sb.TriMesh.FromMesh(tris) as c:
        assert same_bits(a.records, c.records) and same_bits(b.records, c.records)
    empty = np.zeros((0, 3, 6), f32)
    sb.SaveMeshPly(str(tmp_path / "e.ply"), empty)
    assert sb.LoadMeshPly(tmp_path / "e.ply").shape == (0, 3, 6)


def indexed_ply(path, verts6, faces, cut=None):
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n"
            % (len(verts6), len(faces))).encode()
    body = np.asarray(verts6, dtype=f32).tobytes() + b"".join(struct.pack("<B%di" % len(f), len(f), *f) for f in faces)
    data = head + body
    open(path, "wb").write(data if cut is None else data[:cut])
    return len(data)


def test_readers_fan_polygons_and_refuse_broken_files(sb, tmp_path):
    L = sb._lib
    rng = np.random.default_rng(5)
    v = rng.uniform(0, 1, (7, 6)).astype(f32)
    faces = [(0, 1, 2, 3), (2, 3, 4, 5, 6), (6, 0, 1)]
    fan = [(0, 1, 2), (0, 2, 3), (2, 3, 4), (2, 4, 5), (2, 5, 6), (6, 0, 1)]
    want = v[np.array(fan)]
    n = indexed_ply(tmp_path / "i.ply", v, faces)
    assert same_bits(sb.LoadMeshPly(tmp_path / "i.ply"), want)
    # obj: a, a/b, a//c, a/b/c and negative indices; normals from the file where present, else 0
    lines = ["# hand written", "o thing"] + ["v %.9g %.9g %.9g" % tuple(p[:3]) for p in v] + ["vt 0 0"] + \
            ["vn %.9g %.9g %.9g" % tuple(p[3:]) for p in v] + ["s off",
             "f 1 2 3 4", "f 3/1 4/1 5/1 6/1 7/1", "f -1//7 1//1 2//-6", "f 7/1/7 -7/1/-7 2/1/2"]
    open(tmp_path / "i.obj", "w").write("\n".join(lines) + "\n")
    got = sb.LoadMeshObj(tmp_path / "i.obj")
    want_obj = np.concatenate([want, want[5:6]])
    want_obj[:5, :, 3:] = 0
    assert same_bits(got, want_obj)
    # truncated and malformed files
    raw = L.CMesh()
    for cut in (n - 1, n - 14, len(v) * 24 + 200, 30):
        indexed_ply(tmp_path / "t.ply", v, faces, cut)
        assert L.lib.sdfhip_load_ply_mesh(os.fsencode(str(tmp_path / "t.ply")), ctypes.byref(raw)) == L.ERR_IO, cut
        assert not raw.verts6
    indexed_ply(tmp_path / "r.ply", v, [(0, 1, 9)])
    assert L.lib.sdfhip_load_ply_mesh(os.fsencode(str(tmp_path / "r.ply")), ctypes.byref(raw)) == L.ERR_IO
    indexed_ply(tmp_path / "r.ply", v, [(0, 1)])
    assert L.lib.sdfhip_load_ply_mesh(os.fsencode(str(tmp_path / "r.ply")), ctypes.byref(raw)) == L.ERR_IO
    open(tmp_path / "a.ply", "w").write("ply\nformat ascii 1.0\nelement vertex 0\nelement face 0\nend_header\n")
    assert L.lib.sdfhip_load_ply_mesh(os.fsencode(str(tmp_path / "a.ply")), ctypes.byref(raw)) == L.ERR_IO
    assert L.lib.sdfhip_load_ply_mesh(os.fsencode(str(tmp_path / "none.ply")), ctypes.byref(raw)) == L.ERR_IO
    assert L.lib.sdfhip_load_ply_mesh(None, ctypes.byref(raw)) == L.ERR_ARG
    for text in ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n",
                 "v 0 0\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1//1 2//1 3//1\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/x 2 3\n", "g what\n"):
        open(tmp_path / "b.obj", "w").write(text)
        assert L.lib.sdfhip_load_obj_mesh(os.fsencode(str(tmp_path / "b.obj")), ctypes.byref(raw)) == L.ERR_IO, text
    assert L.lib.sdfhip_load_obj_mesh(os.fsencode(str(tmp_path / "none.obj")), ctypes.byref(raw)) == L.ERR_IO

"""Surface extraction (sdfhip_scene_mesh) without a GPU.  The numpy restatement of the rule (tests/mesh_restatement.py; DESIGN.md
section 8, N7) is held here to things it did not make -- the triangle, edge and vertex counts the rule gives on the committed golden
tree, closedness and consistent orientation of the soup, the FROZEN oracle's distance at every vertex, the sphere's outward
direction -- so that tests/test_gpu_mesh.py, which holds the GPU to the restatement byte for byte, is not the builder's code compared
with the builder's code.  And the ABI as far as it goes without a device: names, record sizes, the writers and their round trips
through the project's own readers, the host-only entry points' argument errors."""
import ctypes
import os

import numpy as np
import pytest

import mesh_restatement as mr
from conftest import GOLDEN, bits_equal

f32 = np.float32
MESH_SYMBOLS = ("sdfhip_mesh_options_default", "sdfhip_scene_mesh", "sdfhip_scene_mesh_device", "sdfhip_mesh_free", "sdfhip_mesh_save_ply",
                "sdfhip_mesh_save_obj")


@pytest.fixture(scope="module")
def golden_sphere(sb):
    od = sb.OctData.LoadAsdf(os.path.join(GOLDEN, "sphere_d4.asdf"))
    assert od.Length == 3465
    return od


def test_the_orientation_table_is_a_consistent_surface_of_every_tetrahedron():
    # every (tetrahedron, mask): the right number of triangles, every vertex a cut edge (one end inside, one outside), and a pair of
    # triangles shares its diagonal in opposite directions
    for t in range(6):
        for m in range(16):
            tris = mr.TABLE[t][m]
            assert len(tris) == (0 if m in (0, 15) else 2 if bin(m).count("1") == 2 else 1)
            for tri in tris:
                assert len(set(tri)) == 3
                for i, j in tri:
                    assert i < j and (m >> i & 1) != (m >> j & 1)
            if len(tris) == 2:
                d0 = {(tris[0][k], tris[0][(k + 1) % 3]) for k in range(3)}
                d1 = {(tris[1][(k + 1) % 3], tris[1][k]) for k in range(3)}
                assert len(d0 & d1) == 1
    # the complement mask is the same surface seen from the other side
    for t in range(6):
        for m in range(1, 15):
            a = {frozenset(tri) for tri in mr.TABLE[t][m]}
            b = {frozenset(tri) for tri in mr.TABLE[t][15 - m]}
            if bin(m).count("1") != 2:
                assert a == b
    # Kuhn: the tetrahedra are in the axis permutations' lexicographic order and every edge's lower corner is a subset of the upper
    assert mr.TETS.tolist() == [[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]]
    for tet in mr.TETS:
        for i in range(4):
            for j in range(i + 1, 4):
                assert tet[i] & tet[j] == tet[i]


@pytest.mark.parametrize("level, cut, triangles, edge_count", [(-1, 416, 2520, 3780), (3, 128, 648, 972), (2, 32, 144, 216)])
def test_the_golden_spheres_counts_closedness_and_orientation(golden_sphere, level, cut, triangles, edge_count):
    od = golden_sphere
    tris, nodes, (cells, cells_cut) = mr.mesh(od.Structs, od.Values, level, want_cells=True)
    depth, _ = mr.walk(od.Structs)
    assert cells_cut == cut and len(tris) == triangles
    assert mr.count(od.Structs, od.Values, level) == (cells, cut, triangles)
    if level < 0:
        assert (depth[nodes] == 4).all()                      # all cut cells at depth 4
    else:
        assert (depth[nodes] == level).all()
    assert (np.diff(nodes) >= 0).all()                        # cells in ascending node index
    undirected, not_two, same_way, positions, degenerate = mr.closedness(tris)
    assert undirected == edge_count
    assert not_two == 0, "an edge that does not belong to exactly two triangles"
    assert same_way == 0, "two triangles traverse a shared edge in the same direction"
    assert degenerate == 0
    assert positions - undirected + triangles == 2            # a sphere
    if level < 0:
        assert positions == 1262


def test_a_level_deeper_than_the_tree_is_the_full_mesh_and_level_0_is_the_root(golden_sphere):
    od = golden_sphere
    full = mr.mesh(od.Structs, od.Values, -1)
    for level in (4, 5, 12):
        assert mr.same_bytes(mr.mesh(od.Structs, od.Values, level), full)
    assert mr.count(od.Structs, od.Values, 0) == (1, 0, 0)     # the root's eight corners are all outside
    assert len(mr.mesh(od.Structs, od.Values, 0)) == 0


def cell_bound_bytes(B):
    """Per cell, in byte units: the largest distance between the trilinear interpolant and the linear one along any Kuhn edge.
    With the corner values v[x + 2y + 4z] the trilinear f is linear along a cube edge (0), along a face diagonal it is the linear
    interpolant plus t (1 - t) M, M = the face's mixed second difference (|t (1 - t)| <= 1/4), and along the body diagonal x = y = z = t
    it is the linear interpolant plus (t^2 - t) (Mxy + Mxz + Myz) + (t^3 - t) Mxyz with the mixed differences at corner 0
    (|t^2 - t| <= 1/4, |t^3 - t| <= 2 / (3 sqrt 3))."""
    v = B.astype(np.float64)
    faces = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (2, 3, 6, 7), (0, 2, 4, 6), (1, 3, 5, 7)]
    face = np.max([np.abs(v[:, a] + v[:, d] - v[:, b] - v[:, c]) for a, b, c, d in faces], axis=0) / 4
    mxy = v[:, 3] - v[:, 1] - v[:, 2] + v[:, 0]
    mxz = v[:, 5] - v[:, 1] - v[:, 4] + v[:, 0]
    myz = v[:, 6] - v[:, 2] - v[:, 4] + v[:, 0]
    mxyz = v[:, 7] - v[:, 6] - v[:, 5] - v[:, 3] + v[:, 4] + v[:, 2] + v[:, 1] - v[:, 0]
    body = np.abs(mxy + mxz + myz) / 4 + np.abs(mxyz) * 2 / (3 * np.sqrt(3))
    return np.maximum(face, body)


# fp32 slack of a distance read at a vertex: the position's coordinates are rounded (<= 2^-24 each, positions <= 1), the field
# changes by at most 2 per unit length and axis (a cell's values span at most 2 S over S), and the oracle's own evaluation rounds a
# dozen times on values below 1.5: together below 2^-20
FP32_SLACK = 2.0 ** -20


@pytest.mark.parametrize("name", ["sphere_d4", "torus_d6"])
def test_every_vertex_reads_a_distance_of_zero_within_the_derived_bound(scenes, oracle_mod, name):
    """The oracle's distance at a vertex is the trilinear value there; the vertex is the zero of the LINEAR interpolant along its
    Kuhn edge.  The two differ by at most cell_bound_bytes of the cell, times 2 S / 255 (a byte step as a distance)."""
    od = scenes[name]
    tris, nodes, _ = mr.mesh(od.Structs, od.Values, -1, want_cells=True)
    depth, _ = mr.walk(od.Structs)
    S = 2.0 ** -depth[nodes].astype(np.float64)
    tol = np.repeat(cell_bound_bytes(od.Values[nodes]) * 2 * S / 255 + FP32_SLACK, 3)
    p = tris[:, :, :3].reshape(-1, 3)
    d = np.array([oracle_mod.distance_at(od.Structs, od.Values, *q)[0] for q in p])
    worst = np.abs(d) / np.repeat(S, 3)
    print(f"{name}: {len(p)} vertices, largest |distance| {np.abs(d).max():.3e} = {worst.max():.4f} S; largest bound {tol.max():.3e}; "
          f"largest |distance| / bound {(np.abs(d) / tol).max():.3f}")
    assert (np.abs(d) <= tol).all(), (name, int((np.abs(d) > tol).sum()), float((np.abs(d) / tol).max()))


def test_the_spheres_normals_point_outward_and_the_triangles_face_outward(golden_sphere):
    tris = mr.mesh(golden_sphere.Structs, golden_sphere.Values, -1)
    p, n = tris[:, :, :3].reshape(-1, 3).astype(np.float64), tris[:, :, 3:].reshape(-1, 3).astype(np.float64)
    assert np.isfinite(n).all() and np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5)
    assert (np.einsum("ij,ij->i", n, p - 0.5) > 0).all()
    face = np.cross(tris[:, 1, :3] - tris[:, 0, :3], tris[:, 2, :3] - tris[:, 0, :3]).astype(np.float64)
    assert (np.einsum("ij,ij->i", face, tris[:, 0, :3].astype(np.float64) - 0.5) > 0).all()      # counter-clockwise seen from outside
    r = np.linalg.norm(p - 0.5, axis=1)
    assert abs(r.mean() - 0.3) < 0.01 and r.min() > 0.27 and r.max() < 0.33


def test_the_torus_is_closed_with_euler_characteristic_zero(scenes):
    od = scenes["torus_d6"]
    for level, euler in ((-1, 0), (5, 0), (4, 0)):
        tris = mr.mesh(od.Structs, od.Values, level)
        undirected, not_two, same_way, positions, degenerate = mr.closedness(tris)
        assert len(tris) > 1000 and not_two == 0 and same_way == 0 and degenerate == 0, (level, not_two, same_way)
        assert positions - undirected + len(tris) == euler, level
    assert len(mr.mesh(od.Structs, od.Values, -1)) == 31880


def test_equal_depth_neighbours_produce_the_same_bits_on_shared_edges(scenes):
    # what closedness rests on: a position that two cells produce is the same three words, so keying by bits welds the soup
    od = scenes["torus_d6"]
    tris = mr.mesh(od.Structs, od.Values, -1)
    p = tris[:, :, :3].reshape(-1, 3)
    exact = len(np.unique(p.view(np.uint32).reshape(-1, 3), axis=0))
    rounded = len(np.unique(np.round(p.astype(np.float64) * 2 ** 20).astype(np.int64), axis=0))
    assert exact == rounded == 15940


# ---- the ABI without a device ----------------------------------------------------------------------------------------------

def test_the_library_exports_the_mesh_entry_points_and_record_sizes(sb):
    L = sb._lib
    for name in MESH_SYMBOLS:
        assert hasattr(L.lib, name) and name in L.EXPORTED_SYMBOLS
    assert ctypes.sizeof(L.MeshOptions) == 8 and ctypes.sizeof(L.MeshStats) == 24 and ctypes.sizeof(L.CMesh) == 16
    opt = L.MeshOptions(5)
    opt.size = 0
    L.lib.sdfhip_mesh_options_default(ctypes.byref(opt))
    assert (opt.size, opt.level) == (8, -1)
    L.lib.sdfhip_mesh_options_default(None)                    # a null pointer is not a crash


def test_null_arguments_are_status_codes_and_free_twice_is_safe(sb, tmp_path):
    L = sb._lib
    tris = np.zeros((2, 3, 6), f32)
    raw = L.CMesh(2, tris.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    path = os.fsencode(str(tmp_path / "m.ply"))
    for save in (L.lib.sdfhip_mesh_save_ply, L.lib.sdfhip_mesh_save_obj):
        assert save(ctypes.byref(raw), None) == L.ERR_ARG and L.lib.sdfhip_last_error()
        assert save(None, path) == L.ERR_ARG
        assert save(ctypes.byref(L.CMesh(2, None)), path) == L.ERR_ARG              # triangles and no vertices
        assert save(ctypes.byref(raw), os.fsencode(str(tmp_path / "no" / "such" / "dir.x"))) == L.ERR_IO
    out, st = L.CMesh(), L.MeshStats()
    assert L.lib.sdfhip_scene_mesh(None, None, ctypes.byref(out), ctypes.byref(st)) == L.ERR_ARG
    n = ctypes.c_uint32(7)
    assert L.lib.sdfhip_scene_mesh_device(None, None, None, 0, ctypes.byref(n), None) == L.ERR_ARG
    # sdfhip_mesh_free: what malloc made, twice, and on null
    libc = ctypes.CDLL(None)
    libc.malloc.restype = ctypes.c_void_p
    owned = L.CMesh(1, ctypes.cast(libc.malloc(72), ctypes.POINTER(ctypes.c_float)))
    L.lib.sdfhip_mesh_free(ctypes.byref(owned))
    assert owned.n_triangles == 0 and not owned.verts6
    L.lib.sdfhip_mesh_free(ctypes.byref(owned))
    L.lib.sdfhip_mesh_free(None)


def special_triangles():
    """values a text round trip could lose: denormals, -0, the largest float, NaN normals, nine-digit neighbours"""
    t = np.zeros((3, 3, 6), f32)
    t[0] = np.array([1e-45, -0.0, 3.4028235e38, 1.17549435e-38, 0.1, np.nextafter(f32(0.1), f32(1))], f32)
    t[1, :, 3:] = np.nan
    t[1, :, :3] = np.array([[0.33333334, 0.6666667, 1.0], [0.99999994, 1.0000001, 5e-324], [16777216.0, 16777218.0, -1e-10]], f32)
    t[2] = np.random.default_rng(3).normal(size=(3, 6)).astype(f32)
    return t


@pytest.mark.parametrize("what", ["sphere", "special", "empty"])
def test_ply_and_obj_round_trip_through_the_projects_own_readers(sb, golden_sphere, tmp_path, what):
    tris = {"sphere": lambda: mr.mesh(golden_sphere.Structs, golden_sphere.Values, -1), "special": special_triangles,
            "empty": lambda: np.zeros((0, 3, 6), f32)}[what]()
    flat = tris.reshape(-1, 6)
    ply, obj = str(tmp_path / "mesh.ply"), str(tmp_path / "mesh.obj")
    sb.SaveMeshPly(ply, tris)
    back = sb.OctData.LoadPly(ply)
    assert back.shape == flat.shape and back.tobytes() == flat.tobytes()                  # bit for bit, NaN payloads included
    # the file itself: header, 24 bytes per vertex, then 13 bytes per face {3, 3i, 3i + 1, 3i + 2}
    data = open(ply, "rb").read()
    head, _, body = data.partition(b"end_header\n")
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and f"element vertex {len(flat)}\n".encode() in head
    assert head.index(b"element vertex") < head.index(b"element face") and f"element face {len(tris)}\n".encode() in head
    assert b"property list uchar int vertex_indices" in head
    assert len(body) == 24 * len(flat) + 13 * len(tris)
    faces = np.frombuffer(body[24 * len(flat):], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert (faces["n"] == 3).all() and (faces["v"] == 3 * np.arange(len(tris))[:, None] + np.arange(3)).all()
    sb.SaveMeshObj(obj, tris)
    back = sb.OctData.LoadObj(obj)
    assert back.shape == flat.shape and bits_equal(back, flat).all()                      # %.9g carries every fp32 (NaN as NaN)
    lines = open(obj).read().splitlines()
    assert sum(l.startswith("v ") for l in lines) == len(flat) == sum(l.startswith("vn ") for l in lines)
    assert [l for l in lines if l.startswith("f ")][:1] == (["f 1//1 2//2 3//3"] if len(tris) else [])

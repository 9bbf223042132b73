"""The 1.4 M-node tree of the cell passes' GPU tests (test_gpu_mesh.py, test_gpu_slice.py; test_gpu_measure.py builds the same shape):
1 409 849 nodes are 1377 chunks of 1024, so every thread of the one-workgroup chunk scan owns more than one chunk's total.  The tree
and the mesh restatement's answer at level -1 (11 s of numpy) are made once for every module and both flavours of the library."""
import mesh_restatement as mr

SHAPE = [0.66, 0.5, 0.42, 0.2]      # an off-centre sphere, depth 9
NODES, CELLS, CELLS_CUT, TRIANGLES = 1409849, 1233618, 197656, 1182576

_made = {}


def tree():
    if "tree" not in _made:
        import sdfbox_amd as base
        _made["tree"] = base.OctData.Generate(base._lib.SHAPE_SPHERE, SHAPE, 9)
    return _made["tree"]


def meshed():
    """mr.mesh's (triangles, their nodes, (cells, cut cells)) at level -1"""
    if "mesh" not in _made:
        od = tree()
        _made["mesh"] = mr.mesh(od.Structs, od.Values, -1, want_cells=True, walked=mr.walk(od.Structs))
    return _made["mesh"]

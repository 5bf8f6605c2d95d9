"""Connected components of an indexed triangle mesh on the GPU (er_mesh_components).  The cleaned mesh of a resident volume
is TSDFVolume.extract_clean_mesh (tsdf.py)."""
import ctypes as C

import numpy as np

from . import _ffi


def components(tris, n_vertices, device=0, rounds=False):
    """Labels the mesh of n_vertices vertices and triangles int32[nt, 3]: -> (labels int32[nv] = the smallest vertex index of each vertex's
    component, counts int64[nv] = the triangles of its component, n_components).  A vertex no triangle names is a component of its own with
    0 triangles.  An index outside [0, n_vertices) is refused with the first offending triangle in the message.  rounds = True appends the
    number of labelling rounds the device needed."""
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    nv = int(n_vertices)
    labels = np.empty(max(nv, 0), dtype=np.int32)
    counts = np.empty(max(nv, 0), dtype=np.int64)
    nc, r = C.c_long(0), C.c_int(0)
    _ffi.check(_ffi.lib().er_mesh_components(_ffi.ptr(t), t.shape[0], nv, int(device), _ffi.ptr(labels), _ffi.ptr(counts), C.byref(nc), C.byref(r)),
               "er_mesh_components")
    return (labels, counts, nc.value, r.value) if rounds else (labels, counts, nc.value)

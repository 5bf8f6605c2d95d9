"""Host-side mirror of the reference's Integrate program over the C ABI (include/er_hip.h).

  TSDFVolume    <->  Integrate/TSDFVolume.h:14-69   (ScaleDepth, Integrate, SaveWorld, data_)
  IntegrateApp  <->  Integrate/IntegrateApp.h:33-94 (Init, Execute gating, Reproject) -- same member
                     names as the reference so parity tests read like the reference's own flow.

All arithmetic runs in the HIP kernels of liber_hip.so; this file only marshals buffers and
reproduces the reference's per-frame control flow (frame ids are 1-based, IntegrateApp.cpp:185).
"""
import ctypes as C
import os

import numpy as np

from . import _ffi
from . import formats

UNIT_VOX = 64 * 64 * 64


def mat4_mul(A, B):
    """Row-major 4x4 float64 product in Eigen's coefficient order ((a0*b0 + a1*b1) + a2*b2) + a3*b3."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    out = np.empty((4, 4), np.float64)
    for r in range(4):
        for c in range(4):
            out[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
    return out


class TSDFVolume:
    """TSDFVolume (TSDFVolume.h:14-69) resident in HBM on one GPU."""

    def __init__(self, cols=640, rows=480, camera=None, max_units=1024, device=0):
        self._lib = _ffi.lib()
        self.cols_, self.rows_ = int(cols), int(rows)
        cam = None if camera is None else np.ascontiguousarray(camera, dtype=np.float32)
        self.camera_ = formats.load_camera(None) if cam is None else cam
        self.max_units = int(max_units)
        self.device = int(device)
        h = C.c_void_p()
        _ffi.check(self._lib.er_tsdf_create(self.cols_, self.rows_,
                                            self.camera_.ctypes.data_as(C.POINTER(C.c_float)),
                                            self.max_units, self.device, C.byref(h)), "er_tsdf_create")
        self._h = h
        self.color_enabled_ = False

    def close(self):
        if getattr(self, "_h", None):
            self._lib.er_tsdf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- stream / sync -------------------------------------------------------------------------
    def set_stream(self, hip_stream_ptr):
        _ffi.check(self._lib.er_tsdf_set_stream(self._h, C.c_void_p(hip_stream_ptr)), "er_tsdf_set_stream")

    def synchronize(self):
        _ffi.check(self._lib.er_tsdf_synchronize(self._h), "er_tsdf_synchronize")

    def wait_event(self, hip_event_ptr):
        """The next IntegrateFrames call's pre-pass waits for this hipEvent_t (device depth produced asynchronously)."""
        _ffi.check(self._lib.er_tsdf_wait_event(self._h, C.c_void_p(hip_event_ptr)), "er_tsdf_wait_event")

    def reset(self):
        """data_.clear(): an empty volume in the same buffers."""
        _ffi.check(self._lib.er_tsdf_reset(self._h), "er_tsdf_reset")

    def set_unit_shard(self, rank, world):
        """Unit-shard mode (bit-exact): this volume only owns the units with er_unit_owner(key, world) == rank."""
        _ffi.check(self._lib.er_tsdf_set_unit_shard(self._h, int(rank), int(world)), "er_tsdf_set_unit_shard")

    def status(self):
        """(flags, out_of_range_pixels): sticky overflow flags (ER_STATUS_*) and the pixels skipped beyond +-96 m; a poll."""
        f, n = C.c_int(0), C.c_long(0)
        _ffi.check(self._lib.er_tsdf_status(self._h, C.byref(f), C.byref(n)), "er_tsdf_status")
        return f.value, n.value

    # -- numeric core ---------------------------------------------------------------------------
    def ScaleDepth(self, depth):
        """TSDFVolume::ScaleDepth (TSDFVolume.cpp:19-36)."""
        d = np.ascontiguousarray(depth, dtype=np.uint16).reshape(-1)
        assert d.size == self.cols_ * self.rows_
        out = np.empty(d.size, dtype=np.float32)
        _ffi.check(self._lib.er_tsdf_scale_depth(self._h, _ffi.ptr(d), _ffi.ptr(out)), "er_tsdf_scale_depth")
        return out

    def Reproject(self, depth, ctr, resolution, length, seg, madj):
        """Pixel loop of CIntegrateApp::Reproject (IntegrateApp.cpp:236-268) for one frame; returns the new depth."""
        d = np.array(depth, dtype=np.uint16).reshape(-1)
        g = np.ascontiguousarray(ctr, dtype=np.float32).reshape(-1)
        s = np.ascontiguousarray(seg, dtype=np.float64).reshape(16)
        m = np.ascontiguousarray(madj, dtype=np.float64).reshape(16)
        _ffi.check(self._lib.er_tsdf_reproject(self._h, _ffi.ptr(d), _ffi.ptr(g), int(resolution), C.c_float(length),
                                               _ffi.ptr(s), _ffi.ptr(m)), "er_tsdf_reproject")
        return d

    def Integrate(self, depth, transformation):
        """ScaleDepth + TSDFVolume::Integrate for one frame (IntegrateApp.cpp:224-225)."""
        d = np.ascontiguousarray(depth, dtype=np.uint16).reshape(-1)
        T = np.ascontiguousarray(transformation, dtype=np.float64).reshape(16)
        _ffi.check(self._lib.er_tsdf_integrate(self._h, _ffi.ptr(d), _ffi.ptr(T)), "er_tsdf_integrate")

    @staticmethod
    def _warp_ref(warp, n):
        """The warp dict of IntegrateFrames as (byref(er_warp) or None, the arrays it points into)."""
        if warp is None:
            return None, []
        ctr = np.ascontiguousarray(warp["ctr"], dtype=np.float32)
        gi = np.ascontiguousarray(warp["grid_index"], dtype=np.int32).reshape(-1)
        seg = np.ascontiguousarray(warp["seg"], dtype=np.float64).reshape(-1, 16)
        madj = np.ascontiguousarray(warp["madj"], dtype=np.float64).reshape(-1, 16)
        assert gi.size == n and seg.shape[0] == n and madj.shape[0] == n
        res = int(warp["resolution"])
        num = ctr.size // (3 * (res + 1) ** 3)
        w = _ffi.ErWarp(ctr.ctypes.data_as(C.POINTER(C.c_float)), num, res, C.c_float(warp["length"]),
                        gi.ctypes.data_as(C.POINTER(C.c_int)), seg.ctypes.data_as(C.POINTER(C.c_double)),
                        madj.ctypes.data_as(C.POINTER(C.c_double)))
        return C.byref(w), [ctr, gi, seg, madj, w]

    def IntegrateFrames(self, depth, transformations, warp=None, device_ptr=None):
        """n frames in order.  depth: uint16[n, rows*cols] on the host, or device_ptr = address of the same
        layout in HBM.  warp = dict(ctr=float32[num, verts, 3], resolution, length, grid_index=int[n],
        seg=float64[n,4,4], madj=float64[n,4,4]) or None."""
        T = np.ascontiguousarray(transformations, dtype=np.float64).reshape(-1, 16)
        n = T.shape[0]
        w_ref, keep = self._warp_ref(warp, n)
        if device_ptr is not None:
            _ffi.check(self._lib.er_tsdf_integrate_frames(self._h, n, C.c_void_p(device_ptr), 1, _ffi.ptr(T), w_ref),
                       "er_tsdf_integrate_frames")
        else:
            d = np.ascontiguousarray(depth, dtype=np.uint16).reshape(n, -1)
            assert d.shape[1] == self.cols_ * self.rows_
            _ffi.check(self._lib.er_tsdf_integrate_frames(self._h, n, _ffi.ptr(d), 0, _ffi.ptr(T), w_ref),
                       "er_tsdf_integrate_frames")
        del keep

    def prepass_trace(self, depth, transformations, warp=None, device_ptr=None):
        """er_tsdf_prepass_trace (test hook): IntegrateFrames of ONE batch (<= 64 frames) on a quiet volume, then what its voxel pass was
        given.  Returns dict(scaled float32 [n, pixels + pad], pad, tile_max / tile_lo float32 [tiles_y, tiles_x, n] (32-pixel tiles),
        tile_lo_fine float32 [fine_y, fine_x, n] (16-pixel tiles), keys int32 [k] ascending, masks uint64 [k])."""
        T = np.ascontiguousarray(transformations, dtype=np.float64).reshape(-1, 16)
        n = T.shape[0]
        w_ref, keep = self._warp_ref(warp, n)
        px = self.cols_ * self.rows_
        if device_ptr is not None:
            src, on_dev = C.c_void_p(device_ptr), 1
        else:
            d = np.ascontiguousarray(depth, dtype=np.uint16).reshape(n, -1)
            assert d.shape[1] == px
            src, on_dev = _ffi.ptr(d), 0
        B = 64                                                  # ER_MAX_BATCH
        tx, ty = (self.cols_ + 31) // 32, (self.rows_ + 31) // 32
        fx, fy = (self.cols_ + 15) // 16, (self.rows_ + 15) // 16
        pad, nk = C.c_int(0), C.c_int(0)
        pad_floats = 64                                       # kScaledPad; checked against the library's answer below
        scaled = np.empty((n, px + pad_floats), np.float32)
        tmax, tlo = np.empty((ty, tx, B), np.float32), np.empty((ty, tx, B), np.float32)
        fine = np.empty((fy, fx, B), np.float32)
        cap = 1 << 16
        keys, masks = np.empty(cap, np.int32), np.empty(cap, np.uint64)
        _ffi.check(self._lib.er_tsdf_prepass_trace(self._h, n, src, on_dev, _ffi.ptr(T), w_ref, _ffi.ptr(scaled), C.byref(pad), _ffi.ptr(tmax),
                                                   _ffi.ptr(tlo), _ffi.ptr(fine), _ffi.ptr(keys), _ffi.ptr(masks), cap, C.byref(nk)),
                   "er_tsdf_prepass_trace")
        del keep
        assert pad.value == pad_floats and nk.value <= cap
        return dict(scaled=scaled, pad=pad.value, tile_max=tmax[:, :, :n].copy(), tile_lo=tlo[:, :, :n].copy(),
                    tile_lo_fine=fine[:, :, :n].copy(), keys=keys[:nk.value].copy(), masks=masks[:nk.value].copy())

    def set_zbuf_epoch(self, which, epoch):
        """er_tsdf_set_zbuf_epoch (test hook): the use counter of reprojection z-buffer `which` (0, 1: batch b scatters into b mod 2, Reproject into
        0; 2: the colour calls') as the next use finds it; the buffer refills itself when the counter would pass 0xFFFF."""
        _ffi.check(self._lib.er_tsdf_set_zbuf_epoch(self._h, int(which), int(epoch)), "er_tsdf_set_zbuf_epoch")

    # -- data_ access ---------------------------------------------------------------------------
    def unit_count(self):
        n = C.c_int(0)
        _ffi.check(self._lib.er_tsdf_unit_count(self._h, C.byref(n)), "er_tsdf_unit_count")
        return n.value

    def unit_keys(self):
        n = self.unit_count()
        keys = np.empty(n, dtype=np.int32)
        if n:
            _ffi.check(self._lib.er_tsdf_unit_keys(self._h, _ffi.ptr(keys)), "er_tsdf_unit_keys")
        return keys

    def read_unit(self, key):
        sdf = np.empty(UNIT_VOX, dtype=np.float32)
        w = np.empty(UNIT_VOX, dtype=np.float32)
        _ffi.check(self._lib.er_tsdf_read_unit(self._h, int(key), _ffi.ptr(sdf), _ffi.ptr(w)), "er_tsdf_read_unit")
        return sdf, w

    def sum_weight(self):
        s = C.c_double(0)
        _ffi.check(self._lib.er_tsdf_sum_weight(self._h, C.byref(s)), "er_tsdf_sum_weight")
        return s.value

    def extract_world(self):
        """SaveWorld's point list (TSDFVolume.cpp:104-132) as float32[n, 4] = x y z intensity."""
        n = C.c_long(0)
        _ffi.check(self._lib.er_tsdf_extract_world(self._h, None, 0, C.byref(n)), "er_tsdf_extract_world")
        out = np.empty((n.value, 4), dtype=np.float32)
        if n.value:
            _ffi.check(self._lib.er_tsdf_extract_world(self._h, _ffi.ptr(out), n.value, C.byref(n)), "er_tsdf_extract_world")
        return out

    def extract_surface(self):
        """Zero-crossing points of the volume (er_tsdf_extract_surface) as float32[n, 4] = x y z axis, metres."""
        n = C.c_long(0)
        _ffi.check(self._lib.er_tsdf_extract_surface(self._h, None, 0, C.byref(n)), "er_tsdf_extract_surface")
        out = np.empty((n.value, 4), dtype=np.float32)
        if n.value:
            _ffi.check(self._lib.er_tsdf_extract_surface(self._h, _ffi.ptr(out), n.value, C.byref(n)), "er_tsdf_extract_surface")
        return out

    def extract_oriented(self):
        """extract_surface's list with a normal per point (er_tsdf_extract_oriented): (points float32[n, 4] = x y z axis, normals float32[n, 3]).
        The normal is the normalised central difference of the sdf at the point's nearest voxel; a row is NaN where that voxel or one of its
        six neighbours was never observed (what the kinfu fragment step leaves in cloud_bin_<i>.pcd, CorresApp.cpp:93-98 filters)."""
        n = C.c_long(0)
        _ffi.check(self._lib.er_tsdf_extract_oriented(self._h, None, None, 0, C.byref(n)), "er_tsdf_extract_oriented")
        pts = np.empty((n.value, 4), dtype=np.float32)
        nrm = np.empty((n.value, 4), dtype=np.float32)
        if n.value:
            _ffi.check(self._lib.er_tsdf_extract_oriented(self._h, _ffi.ptr(pts), _ffi.ptr(nrm), n.value, C.byref(n)), "er_tsdf_extract_oriented")
        return pts, np.ascontiguousarray(nrm[:, :3])

    def raycast(self, T, cols=None, rows=None, cam=None, levels=1, params=None, device=False):
        """er_tsdf_raycast from the pose T (world_T_camera, 4 x 4 float64): per level l = 0 .. levels - 1 a tuple (depth uint16 [r, c] in
        millimetres, vertex map float32 [r, c, 3], normal map float32 [r, c, 3]) of the image cols / 2^l x rows / 2^l with cam / 2^l, camera
        frame, NaN / 0 where the ray meets no surface.  cols, rows, cam = (fx, fy, cx, cy) default to the volume's own image;
        params = (t_min, t_max, step) in metres, None = er_raycast_params_default.  device = True: torch tensors on the volume's GPU, the
        two maps as views of ONE record tensor [r, c, 2, 4] -- er_odom's record layout, what DepthOdometry.align_model reads in place."""
        cols = self.cols_ if cols is None else int(cols)
        rows = self.rows_ if rows is None else int(rows)
        cam4 = np.ascontiguousarray(np.asarray(self.camera_ if cam is None else cam, np.float32).reshape(-1)[:4])
        levels = int(levels)
        if levels < 1 or cols % (1 << (levels - 1)) or rows % (1 << (levels - 1)):
            raise ValueError("raycast: %d x %d is not divisible by 2^(levels-1), levels = %d" % (cols, rows, levels))
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        P = None
        if params is not None:
            P = C.byref(_ffi.ErRaycastParams(*[float(np.float32(x)) for x in params]))
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            torch.cuda.current_stream(dev).synchronize()         # (the tensors' memory may have work of torch's stream pending on it)
        out = []
        for l in range(levels):
            c, r = cols >> l, rows >> l
            k = np.ascontiguousarray(cam4 / np.float32(1 << l))
            if device:
                rec = torch.empty((r, c, 2, 4), dtype=torch.float32, device=dev)
                dep = torch.empty((r, c), dtype=torch.uint16, device=dev)
                rp, dp = C.c_void_p(rec.data_ptr()), C.c_void_p(dep.data_ptr())
            else:
                rec, dep = np.empty((r, c, 2, 4), np.float32), np.empty((r, c), np.uint16)
                rp, dp = _ffi.ptr(rec), _ffi.ptr(dep)
            _ffi.check(self._lib.er_tsdf_raycast(self._h, c, r, _ffi.ptr(k), _ffi.ptr(T), P, rp, dp, 1 if device else 0), "er_tsdf_raycast")
            if device:
                out.append((dep, rec[:, :, 0, :3], rec[:, :, 1, :3]))
            else:
                out.append((dep, np.ascontiguousarray(rec[:, :, 0, :3]), np.ascontiguousarray(rec[:, :, 1, :3])))
        return out

    def SaveFragment(self, filename, length=3.0):
        """cloud_bin_<i>.pcd of the resident volume: the oriented points inside the cube 0 <= x, y, z < length (PointCloud::GetCoordinate's cube),
        NaN-normal rows KEPT -- CCorresApp::LoadData filters them (CorresApp.cpp:93-98).  Returns the number of points written."""
        pts, nrm = self.extract_oriented()
        x = pts[:, :3]
        inside = ((x >= np.float32(0.0)) & (x < np.float32(length))).all(axis=1)
        formats.save_pcd_xyzn(filename, np.ascontiguousarray(x[inside]), np.ascontiguousarray(nrm[inside]))
        return int(inside.sum())

    def extract_mesh(self):
        """Marching-cubes triangles of the volume (er_tsdf_extract_mesh) as float32[n, 3, 3] = triangle, vertex, xyz in metres."""
        n = C.c_long(0)
        _ffi.check(self._lib.er_tsdf_extract_mesh(self._h, None, 0, C.byref(n)), "er_tsdf_extract_mesh")
        out = np.empty((n.value, 3, 3), dtype=np.float32)
        if n.value:
            _ffi.check(self._lib.er_tsdf_extract_mesh(self._h, _ffi.ptr(out), n.value, C.byref(n)), "er_tsdf_extract_mesh")
        return out

    def SaveWorld(self, filename):
        pts = self.extract_world()
        formats.save_pcd_xyzi(filename, pts)
        return pts.shape[0]

    def extract_indexed_mesh(self, colors=False):
        """extract_mesh's triangles as an indexed mesh (er_tsdf_extract_mesh_indexed): (verts float32[n, 4] = x y z axis, normals float32[n, 3],
        tris int32[m, 3]).  A vertex is a lattice edge that a triangle uses, in extract_surface's order; verts[tris][..., :3] is extract_mesh's
        soup bit for bit; a normal is extract_oriented's rule at the vertex, NaN where it gives none.  colors = True appends sample_colors(verts),
        uint8[n, 4]."""
        nv, nt = C.c_long(0), C.c_long(0)
        _ffi.check(self._lib.er_tsdf_extract_mesh_indexed(self._h, None, None, 0, None, 0, C.byref(nv), C.byref(nt)), "er_tsdf_extract_mesh_indexed")
        verts = np.empty((nv.value, 4), dtype=np.float32)
        nrm = np.empty((nv.value, 4), dtype=np.float32)
        tris = np.empty((nt.value, 3), dtype=np.int32)
        if nv.value:
            _ffi.check(self._lib.er_tsdf_extract_mesh_indexed(self._h, _ffi.ptr(verts), _ffi.ptr(nrm), nv.value, _ffi.ptr(tris), nt.value,
                                                              C.byref(nv), C.byref(nt)), "er_tsdf_extract_mesh_indexed")
        if colors:
            return verts, np.ascontiguousarray(nrm[:, :3]), tris, self.sample_colors(verts)
        return verts, np.ascontiguousarray(nrm[:, :3]), tris

    def extract_clean_mesh(self, min_triangles=0, largest_only=False, colors=False, stats=False):
        """extract_indexed_mesh without its small connected components (er_tsdf_extract_mesh_cleaned; the unfiltered mesh never leaves the
        device): (verts, normals, tris, index[, rgba][, stats]) in extract_indexed_mesh's layouts.  A component -- vertices joined by
        triangles -- is kept iff it has at least min_triangles triangles and, with largest_only, is the one with the most (a tie goes to the
        one that holds the lowest vertex); kept vertices and triangles keep their order, index int32[n] is each kept vertex's position in the
        unfiltered mesh.  colors = True appends sample_colors(verts); stats = True appends (components found, components kept, vertices
        dropped, triangles dropped)."""
        nv, nt = C.c_long(0), C.c_long(0)
        st = (C.c_long * 4)(0, 0, 0, 0)
        call = self._lib.er_tsdf_extract_mesh_cleaned
        _ffi.check(call(self._h, int(min_triangles), int(bool(largest_only)), None, None, None, 0, None, 0, C.byref(nv), C.byref(nt), st),
                   "er_tsdf_extract_mesh_cleaned")
        verts = np.empty((nv.value, 4), dtype=np.float32)
        nrm = np.empty((nv.value, 4), dtype=np.float32)
        index = np.empty(nv.value, dtype=np.int32)
        tris = np.empty((nt.value, 3), dtype=np.int32)
        if nv.value:
            _ffi.check(call(self._h, int(min_triangles), int(bool(largest_only)), _ffi.ptr(verts), _ffi.ptr(nrm), _ffi.ptr(index), nv.value,
                            _ffi.ptr(tris), nt.value, C.byref(nv), C.byref(nt), st), "er_tsdf_extract_mesh_cleaned")
        out = (verts, np.ascontiguousarray(nrm[:, :3]), tris, index)
        if colors:
            out += (self.sample_colors(verts),)
        if stats:
            out += ((st[0], st[1], st[2], st[3]),)
        return out

    def extract_simplified_mesh(self, cell, min_triangles=0, largest_only=False, colors=False, stats=False):
        """The mesh of the resident volume simplified by vertex clustering (er_tsdf_extract_mesh_simplified; the unsimplified
        mesh never leaves the device): (verts float32[n, 4] = x y z 0, normals float32[n, 3], tris int32[m, 3][, rgba][, stats]).  The mesh that
        is clustered is extract_indexed_mesh's or, with min_triangles > 1 or largest_only, extract_clean_mesh's; the result is
        mesh.simplify(verts, tris, cell, normals, colors) of it, where colors = True samples the unsimplified vertices (sample_colors) and
        averages them per cluster.  cell is in metres.  stats = True appends (occupied cells, degenerate triangles dropped, duplicates dropped,
        cells dropped, vertices before, triangles before)."""
        nv, nt = C.c_long(0), C.c_long(0)
        st, before = (C.c_long * 4)(0, 0, 0, 0), (C.c_long * 2)(0, 0)
        call = self._lib.er_tsdf_extract_mesh_simplified
        head = (self._h, C.c_float(cell), int(min_triangles), int(bool(largest_only)), int(bool(colors)))
        _ffi.check(call(*head, None, None, None, None, 0, None, 0, C.byref(nv), C.byref(nt), st, before, None), "er_tsdf_extract_mesh_simplified")
        verts = np.zeros((nv.value, 4), dtype=np.float32)
        nrm = np.zeros((nv.value, 4), dtype=np.float32)
        rgba = np.zeros((nv.value, 4), dtype=np.uint8)
        tris = np.zeros((nt.value, 3), dtype=np.int32)
        if nv.value:
            _ffi.check(call(*head, _ffi.ptr(verts), _ffi.ptr(nrm), _ffi.ptr(rgba) if colors else None, None, nv.value, _ffi.ptr(tris), nt.value,
                            C.byref(nv), C.byref(nt), st, before, None), "er_tsdf_extract_mesh_simplified")
        out = (verts, np.ascontiguousarray(nrm[:, :3]), tris)
        if colors:
            out += (rgba,)
        if stats:
            out += ((st[0], st[1], st[2], st[3], before[0], before[1]),)
        return out

    def extract_smoothed_mesh(self, iterations, lam=0.5, mu=-0.53, fix_boundary=False, cell=0.0, min_triangles=0, largest_only=False, colors=False,
                              stats=False):
        """The mesh of the resident volume after Taubin smoothing (er_tsdf_extract_mesh_smoothed; no intermediate mesh leaves
        the device): (verts float32[n, 4], normals float32[n, 3], tris int32[m, 3][, rgba][, stats]).  The mesh that is smoothed is
        extract_indexed_mesh's or, with min_triangles > 1 or largest_only, extract_clean_mesh's; the result is mesh.smooth(verts, tris,
        iterations, lam, mu, fix_boundary) of it -- positions x y z 0 and the normals of the smoothed triangles -- and, with cell > 0,
        mesh.simplify(.., cell, ..) of that.  colors = True samples the UNSMOOTHED vertices (sample_colors), where the surface was observed.
        iterations = 0 skips the smoothing: the arrays are those of extract_indexed_mesh, extract_clean_mesh or extract_simplified_mesh.
        stats = True appends (distinct edges, boundary edges, non-manifold edges, vertices that never move, then the four of
        extract_simplified_mesh, vertices before, triangles before)."""
        nv, nt = C.c_long(0), C.c_long(0)
        ss, cs, before = (C.c_long * 4)(0, 0, 0, 0), (C.c_long * 4)(0, 0, 0, 0), (C.c_long * 2)(0, 0)
        call = self._lib.er_tsdf_extract_mesh_smoothed
        head = (self._h, int(iterations), C.c_float(lam), C.c_float(mu), int(bool(fix_boundary)), C.c_float(cell), int(min_triangles), int(bool(largest_only)),
                int(bool(colors)))
        first = (ss, cs, before) if cell != 0 else (None, None, None)       # (without the clustering the counts need no smoothing)
        _ffi.check(call(*head, None, None, None, 0, None, 0, C.byref(nv), C.byref(nt), *first), "er_tsdf_extract_mesh_smoothed")
        verts = np.zeros((nv.value, 4), dtype=np.float32)
        nrm = np.zeros((nv.value, 4), dtype=np.float32)
        rgba = np.zeros((nv.value, 4), dtype=np.uint8)
        tris = np.zeros((nt.value, 3), dtype=np.int32)
        if nv.value:
            _ffi.check(call(*head, _ffi.ptr(verts), _ffi.ptr(nrm), _ffi.ptr(rgba) if colors else None, nv.value, _ffi.ptr(tris), nt.value,
                            C.byref(nv), C.byref(nt), ss, cs, before), "er_tsdf_extract_mesh_smoothed")
        out = (verts, np.ascontiguousarray(nrm[:, :3]), tris)
        if colors:
            out += (rgba,)
        if stats:
            out += ((ss[0], ss[1], ss[2], ss[3], cs[0], cs[1], cs[2], cs[3], before[0], before[1]),)
        return out

    def SaveMesh(self, filename, normals=True, binary=True, colors=None, min_triangles=0, largest_only=False, cell=0.0, smooth=0, smooth_lambda=0.5,
                 smooth_mu=-0.53, smooth_fix_boundary=False):
        """The indexed mesh of the resident volume as PLY (formats.save_ply; NaN normals become 0 0 0).  colors = None: per-vertex colours iff
        colour is enabled on the volume; False suppresses them; True demands them.  min_triangles > 1 or largest_only: the cleaned mesh of
        extract_clean_mesh.  cell > 0: that mesh simplified by vertex clustering with cells of `cell` metres (extract_simplified_mesh); 0 writes
        the unsimplified mesh.  smooth > 0: that many Taubin iterations (extract_smoothed_mesh) after the cleaning and before the clustering.
        Returns (vertices, triangles)."""
        if colors is None:
            colors = self.color_enabled_
        if smooth != 0:
            got = self.extract_smoothed_mesh(smooth, smooth_lambda, smooth_mu, smooth_fix_boundary, cell, min_triangles, largest_only, colors=bool(colors))
            verts, nrm, tris, rgba = got[0], got[1], got[2], (got[3] if colors else None)
        elif cell != 0:
            got = self.extract_simplified_mesh(cell, min_triangles, largest_only, colors=bool(colors))
            verts, nrm, tris, rgba = got[0], got[1], got[2], (got[3] if colors else None)
        elif min_triangles > 1 or largest_only:
            got = self.extract_clean_mesh(min_triangles, largest_only, colors=bool(colors))
            verts, nrm, tris, rgba = got[0], got[1], got[2], (got[4] if colors else None)
        elif colors:
            verts, nrm, tris, rgba = self.extract_indexed_mesh(colors=True)
        else:
            (verts, nrm, tris), rgba = self.extract_indexed_mesh(), None
        formats.save_ply(filename, verts, tris, nrm if normals else None, binary, colors=rgba)
        return verts.shape[0], tris.shape[0]

    # -- colour -----------------------------------------------------------------
    def enable_color(self):
        """er_tsdf_color_enable: allocates the per-voxel colour accumulators (4 MiB per unit of max_units).  Idempotent."""
        _ffi.check(self._lib.er_tsdf_color_enable(self._h), "er_tsdf_color_enable")
        self.color_enabled_ = True

    def ColorFrames(self, depth, rgb, transformations, warp=None, device_ptrs=None):
        """er_tsdf_color_frames: splats the colour of n frames -- IntegrateFrames' depth, transformations and warp of the same frames, which are
        meant to have been integrated already -- into the accumulators.  depth: uint16[n, rows*cols], rgb: uint8[n, rows*cols, 3] on the host, or
        device_ptrs = (depth address, rgb address) of the same layouts in HBM.  Returns (added, no_unit, out_of_range) pixels."""
        T = np.ascontiguousarray(transformations, dtype=np.float64).reshape(-1, 16)
        n = T.shape[0]
        w_ref, keep = self._warp_ref(warp, n)
        st = (C.c_long * 3)(0, 0, 0)
        if device_ptrs is not None:
            dp, cp, on_dev = C.c_void_p(device_ptrs[0]), C.c_void_p(device_ptrs[1]), 1
        else:
            d = np.ascontiguousarray(depth, dtype=np.uint16).reshape(-1)
            c = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1)
            if d.size != n * self.cols_ * self.rows_ or c.size != 3 * d.size:
                raise ValueError("ColorFrames: %d depth pixels and %d colour bytes are not %d frames of a %d x %d image"
                                 % (d.size, c.size, n, self.cols_, self.rows_))
            dp, cp, on_dev = _ffi.ptr(d), _ffi.ptr(c), 0
        _ffi.check(self._lib.er_tsdf_color_frames(self._h, n, dp, cp, on_dev, _ffi.ptr(T), w_ref, st), "er_tsdf_color_frames")
        del keep
        return st[0], st[1], st[2]

    def ReprojectColor(self, depth, rgb, ctr, resolution, length, seg, madj):
        """Reproject with the colour image (er_tsdf_reproject_color) for one frame; returns (the new depth, the new colour uint8[rows*cols, 3])."""
        d = np.array(depth, dtype=np.uint16).reshape(-1)
        c = np.array(rgb, dtype=np.uint8).reshape(-1, 3)
        assert d.size == self.cols_ * self.rows_ and c.shape[0] == d.size
        g = np.ascontiguousarray(ctr, dtype=np.float32).reshape(-1)
        s = np.ascontiguousarray(seg, dtype=np.float64).reshape(16)
        m = np.ascontiguousarray(madj, dtype=np.float64).reshape(16)
        _ffi.check(self._lib.er_tsdf_reproject_color(self._h, _ffi.ptr(d), _ffi.ptr(c), _ffi.ptr(g), int(resolution), C.c_float(length),
                                                     _ffi.ptr(s), _ffi.ptr(m)), "er_tsdf_reproject_color")
        return d, c

    def read_unit_color(self, key):
        """The accumulators of one unit: uint32[64^3, 4] = r_sum, g_sum, b_sum, n per voxel, in read_unit's voxel order."""
        a = np.empty((UNIT_VOX, 4), dtype=np.uint32)
        _ffi.check(self._lib.er_tsdf_read_unit_color(self._h, int(key), _ffi.ptr(a)), "er_tsdf_read_unit_color")
        return a

    def write_unit_color(self, key, rgbn):
        a = np.ascontiguousarray(rgbn, dtype=np.uint32).reshape(UNIT_VOX, 4)
        _ffi.check(self._lib.er_tsdf_write_unit_color(self._h, int(key), _ffi.ptr(a)), "er_tsdf_write_unit_color")

    def sample_colors(self, points, counts=False):
        """er_tsdf_sample_colors: uint8[n, 4] = r g b a for points float32[n, 3] or [n, 4] (x y z in metres; a fourth column is ignored), a = 255
        where the nearest voxel (level 0) or its 3 x 3 x 3 neighbourhood (level 1) holds a sample, 0 0 0 0 elsewhere.  counts = True: also
        (points coloured at level 0, at level 1)."""
        p = np.asarray(points, np.float32)
        if p.ndim != 2 or p.shape[1] not in (3, 4):
            raise ValueError("sample_colors: points must be [n, 3] or [n, 4], not %s" % (p.shape,))
        if p.shape[1] == 3:
            p = np.concatenate([p, np.zeros((p.shape[0], 1), np.float32)], axis=1)
        p = np.ascontiguousarray(p)
        out = np.zeros((p.shape[0], 4), dtype=np.uint8)
        ct = (C.c_long * 2)(0, 0)
        _ffi.check(self._lib.er_tsdf_sample_colors(self._h, _ffi.ptr(p), p.shape[0], _ffi.ptr(out), ct), "er_tsdf_sample_colors")
        return (out, (ct[0], ct[1])) if counts else out

    def LoadWorld(self, path_or_array):
        """SaveWorld's inverse (er_tsdf_import_world) into this EMPTY volume: a world.pcd path, or float32[n, 4] = x y z intensity rows as
        extract_world returns them.  Every listed voxel becomes (intensity, weight 1) -- the file carries no weights, 1 marks "observed".
        Returns the number of units created; after a refusal the volume is empty."""
        if isinstance(path_or_array, (str, bytes, os.PathLike)):
            f = formats.load_pcd(path_or_array)
            a = np.stack([np.asarray(f[k], np.float32).reshape(-1) for k in ("x", "y", "z", "intensity")], axis=1)
        else:
            a = np.asarray(path_or_array, np.float32)
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4)
        nu = C.c_int(0)
        _ffi.check(self._lib.er_tsdf_import_world(self._h, _ffi.ptr(a), a.shape[0], C.byref(nu)), "er_tsdf_import_world")
        return nu.value

    # -- multi-GPU frame split ----------------------------------------------------
    def export_weighted(self, keys, dev_ptr):
        k = np.ascontiguousarray(keys, dtype=np.int32)
        _ffi.check(self._lib.er_tsdf_export_weighted(self._h, _ffi.ptr(k), k.size, C.c_void_p(dev_ptr)), "er_tsdf_export_weighted")

    def import_weighted(self, keys, dev_ptr):
        k = np.ascontiguousarray(keys, dtype=np.int32)
        _ffi.check(self._lib.er_tsdf_import_weighted(self._h, _ffi.ptr(k), k.size, C.c_void_p(dev_ptr)), "er_tsdf_import_weighted")

    def export_raw(self, keys, dev_ptr):
        """[key][sdf | weight] planes, bit for bit: how a unit only one GPU touched travels (er_tsdf_export_raw)."""
        k = np.ascontiguousarray(keys, dtype=np.int32)
        _ffi.check(self._lib.er_tsdf_export_raw(self._h, _ffi.ptr(k), k.size, C.c_void_p(dev_ptr)), "er_tsdf_export_raw")

    def import_raw(self, keys, dev_ptr):
        k = np.ascontiguousarray(keys, dtype=np.int32)
        _ffi.check(self._lib.er_tsdf_import_raw(self._h, _ffi.ptr(k), k.size, C.c_void_p(dev_ptr)), "er_tsdf_import_raw")

    # band records (round 6, the owner merge): a unit as its observed voxels only -- include/er_hip.h
    def band_sizes(self, keys):
        """Record size in 32-bit words of each of the given units (er_tsdf_band_sizes)."""
        k = np.ascontiguousarray(keys, dtype=np.int32)
        out = np.zeros(k.size, np.int32)
        _ffi.check(self._lib.er_tsdf_band_sizes(self._h, _ffi.ptr(k), k.size, _ffi.ptr(out)), "er_tsdf_band_sizes")
        return out

    def export_band(self, keys, counts, dev_ptr):
        k, c = np.ascontiguousarray(keys, dtype=np.int32), np.ascontiguousarray(counts, dtype=np.int32)
        _ffi.check(self._lib.er_tsdf_export_band(self._h, _ffi.ptr(k), _ffi.ptr(c), k.size, C.c_void_p(dev_ptr)), "er_tsdf_export_band")

    def import_band(self, keys, rec_ptrs):
        k = np.ascontiguousarray(keys, dtype=np.int32)
        r = (C.c_void_p * k.size)(*[int(p) for p in rec_ptrs])
        _ffi.check(self._lib.er_tsdf_import_band(self._h, _ffi.ptr(k), k.size, r), "er_tsdf_import_band")

    def merge_band(self, keys, srcs, self_pos):
        """srcs[u] = device pointers of the other touchers' records of unit keys[u] in rank order; self_pos[u] of them come before this volume's own voxels."""
        k = np.ascontiguousarray(keys, dtype=np.int32)
        ns = np.asarray([len(x) for x in srcs], np.int32)
        sp = np.ascontiguousarray(self_pos, dtype=np.int32)
        r = (C.c_void_p * (16 * k.size))()
        for u, x in enumerate(srcs):
            for q, ptr in enumerate(x[:16]):                       # (more than 16: the library refuses the call by the count)
                r[16 * u + q] = int(ptr)
        _ffi.check(self._lib.er_tsdf_merge_band(self._h, _ffi.ptr(k), k.size, _ffi.ptr(ns), _ffi.ptr(sp), r), "er_tsdf_merge_band")

    def drop_units(self, keys):
        k = np.ascontiguousarray(keys, dtype=np.int32)
        _ffi.check(self._lib.er_tsdf_drop_units(self._h, _ffi.ptr(k), k.size), "er_tsdf_drop_units")

    # -- profiling --------------------------------------------------------------------------------
    def set_profiling(self, enable):
        """True / 1: time every k_integrate launch; n > 1: every n-th launch; False / 0: off."""
        _ffi.check(self._lib.er_tsdf_set_profiling(self._h, int(enable)), "er_tsdf_set_profiling")

    def get_profile(self):
        ms, ln, fr, uv = C.c_double(0), C.c_long(0), C.c_long(0), C.c_long(0)
        _ffi.check(self._lib.er_tsdf_get_profile(self._h, C.byref(ms), C.byref(ln), C.byref(fr), C.byref(uv)), "er_tsdf_get_profile")
        return {"integrate_ms": ms.value, "launches": ln.value, "frames": fr.value, "unit_visits": uv.value}

    TIMELINE_COLUMNS = ("host_in", "host_consts", "host_out", "x_wait", "x_consts", "x_fix", "x_prepare", "x_plan", "v_begin", "v_end")

    def set_timeline(self, on):
        """er_tsdf_set_timeline: record host and device times of every batch (include/er_hip.h); off by default."""
        _ffi.check(self._lib.er_tsdf_set_timeline(self._h, int(bool(on))), "er_tsdf_set_timeline")

    def get_timeline(self):
        """er_tsdf_get_timeline: waits for the recorded batches and returns one dict per batch, in order -- batch, slot, stream, frames and
        the TIMELINE_COLUMNS in ms since set_timeline(True); clears the record."""
        n = C.c_int(0)
        _ffi.check(self._lib.er_tsdf_get_timeline(self._h, 0, None, None, C.byref(n)), "er_tsdf_get_timeline")
        meta = np.zeros((max(n.value, 1), 4), np.int64)
        t = np.zeros((max(n.value, 1), len(self.TIMELINE_COLUMNS)), np.float64)
        _ffi.check(self._lib.er_tsdf_get_timeline(self._h, n.value, _ffi.ptr(meta), _ffi.ptr(t), C.byref(n)), "er_tsdf_get_timeline")
        return [dict(batch=int(m[0]), slot=int(m[1]), stream=int(m[2]), frames=int(m[3]), **dict(zip(self.TIMELINE_COLUMNS, map(float, r))))
                for m, r in zip(meta[:n.value], t[:n.value])]


def raycast_batch(jobs, depth=True):
    """er_tsdf_raycast_batch: a list of ray-casts in ONE launch.  jobs: dicts (or tuples in this order) of volume (a TSDFVolume), T
    (world_T_camera), cols, rows, cam = (fx, fy, cx, cy) and optionally params = (t_min, t_max, step); all volumes on one device.  Returns
    per job (depth uint16 [r, c] or None, vertex map [r, c, 3], normal map [r, c, 3]) as torch tensors on that device, the two maps views
    of one record tensor [r, c, 2, 4] as TSDFVolume.raycast(device = True) returns them -- and the same bits.  depth = False: no depth image."""
    import torch
    lib = _ffi.lib()
    keys = ("volume", "T", "cols", "rows", "cam", "params")
    jobs = [j if isinstance(j, dict) else dict(zip(keys, j)) for j in jobs]
    n = len(jobs)
    if n == 0:
        _ffi.check(lib.er_tsdf_raycast_batch(0, None, None, None, None, None, None, None, None), "er_tsdf_raycast_batch")
        return []
    dev = torch.device("cuda", jobs[0]["volume"].device)
    vols = (C.c_void_p * n)(*[j["volume"]._h.value for j in jobs])
    cols = np.array([int(j["cols"]) for j in jobs], np.int32)
    rows = np.array([int(j["rows"]) for j in jobs], np.int32)
    cam = np.ascontiguousarray([np.asarray(j["cam"], np.float32).reshape(-1)[:4] for j in jobs], dtype=np.float32)
    T = np.ascontiguousarray([np.asarray(j["T"], np.float64).reshape(16) for j in jobs], dtype=np.float64)
    P = None
    if any(j.get("params") is not None for j in jobs):
        d = _ffi.ErRaycastParams()
        _ffi.check(lib.er_raycast_params_default(C.byref(d)), "er_raycast_params_default")
        P = (_ffi.ErRaycastParams * n)()
        for q, j in enumerate(jobs):
            P[q] = d if j.get("params") is None else _ffi.ErRaycastParams(*[float(np.float32(x)) for x in j["params"]])
    recs = [torch.empty((max(int(r), 0), max(int(c), 0), 2, 4), dtype=torch.float32, device=dev) for c, r in zip(cols, rows)]
    deps = [torch.empty((max(int(r), 0), max(int(c), 0)), dtype=torch.uint16, device=dev) if depth else None for c, r in zip(cols, rows)]
    torch.cuda.current_stream(dev).synchronize()                 # (the tensors' memory may have work of torch's stream pending on it)
    rp = (C.c_void_p * n)(*[t.data_ptr() for t in recs])
    dp = (C.c_void_p * n)(*[t.data_ptr() for t in deps]) if depth else None
    _ffi.check(lib.er_tsdf_raycast_batch(n, vols, _ffi.ptr(cols), _ffi.ptr(rows), _ffi.ptr(cam), _ffi.ptr(T), P, rp, dp), "er_tsdf_raycast_batch")
    return [(deps[q], recs[q][:, :, 0, :3], recs[q][:, :, 1, :3]) for q in range(n)]


class IntegrateApp:
    """CIntegrateApp (IntegrateApp.h:33-94) without the OpenNI grabber: frames are fed by the caller.

    Member names follow the reference.  Execute() reproduces the per-frame gating of
    IntegrateApp.cpp:190-226 exactly (including its quirks); frames that pass
    the gates are queued and flushed to the GPU in batches -- the results equal frame-by-frame
    execution because the device processes a batch in frame order per voxel.
    """

    def __init__(self, cols=640, rows=480, max_units=1024, device=0, batch=64):
        self.cols_, self.rows_ = cols, rows
        self.traj_filename_ = ""
        self.pose_filename_ = ""
        self.seg_filename_ = ""
        self.camera_filename_ = ""
        self.ctr_filename_ = ""
        self.pcd_filename_ = "world.pcd"
        self.ctr_num_ = 0
        self.ctr_resolution_ = 8
        self.ctr_interval_ = 50
        self.ctr_length_ = 3.0
        self.start_from_ = -1
        self.end_at_ = 100000000
        self.exit_ = False
        self.frame_id_ = 0
        self.traj_ = []
        self.seg_traj_ = []
        self.pose_traj_ = []
        self.grids_ = None
        self.volume_ = None
        self._max_units, self._device, self._batch = max_units, device, int(batch)
        self._q_depth, self._q_T, self._q_gi, self._q_seg, self._q_madj = [], [], [], [], []
        self._q_color = []
        self.frames_integrated = 0

    def Init(self):
        """CIntegrateApp::Init (IntegrateApp.cpp:43-79)."""
        import os
        camera = formats.load_camera(self.camera_filename_ if os.path.exists(self.camera_filename_ or "") else None)
        self.volume_ = TSDFVolume(self.cols_, self.rows_, camera, self._max_units, self._device)
        if self.ctr_num_ > 0 and os.path.exists(self.ctr_filename_ or "") and os.path.exists(self.seg_filename_ or ""):
            self.grids_ = formats.load_ctr(self.ctr_filename_, self.ctr_num_, self.ctr_resolution_)
        else:
            self.ctr_num_ = 0
        if os.path.exists(self.traj_filename_ or ""):
            self.traj_ = formats.load_log(self.traj_filename_)
        if os.path.exists(self.seg_filename_ or ""):
            self.seg_traj_ = formats.load_log(self.seg_filename_)
            if os.path.exists(self.pose_filename_ or ""):
                self.pose_traj_ = formats.load_log(self.pose_filename_)
                self.traj_ = []
                for i in range(len(self.pose_traj_)):
                    for j in range(self.ctr_interval_):
                        idx = i * self.ctr_interval_ + j
                        self.traj_.append(formats.FramedTransformation(
                            idx, idx, idx + 1, mat4_mul(self.pose_traj_[i].T, self.seg_traj_[idx].T)))

    def Execute(self, frame_id, depth, color=None):
        """One main-loop turn with data (IntegrateApp.cpp:190-226); frame_id is 1-based.  color: the frame's registered colour image,
        uint8[rows, cols, 3], or None -- with colour, every frame of the run must carry one; the colour of each batch is splatted behind
        its integration (bin/Integrate --color_raw / --color_list)."""
        self.frame_id_ = frame_id
        if self.traj_[frame_id - 1].frame == -1:
            return
        if frame_id >= len(self.traj_):
            self.exit_ = True
            return
        if frame_id < self.start_from_ or frame_id > self.end_at_:
            if frame_id > self.end_at_:
                self.exit_ = True
            return
        T = self.traj_[frame_id - 1].T
        if self.ctr_num_ > 0:
            if frame_id > self.ctr_interval_ * self.ctr_num_:          # Reproject, IntegrateApp.cpp:230-233
                self.exit_ = True
                return
            chunk = (frame_id - 1) // self.ctr_interval_
            madj = mat4_mul(mat4_mul(_inverse(T), self.traj_[0].T), _inverse(self.seg_traj_[0].T))
            self._q_gi.append(chunk)
            self._q_seg.append(self.seg_traj_[frame_id - 1].T.copy())
            self._q_madj.append(madj)
        self._q_depth.append(np.ascontiguousarray(depth, dtype=np.uint16).reshape(-1))
        if color is not None:
            self._q_color.append(np.ascontiguousarray(color, dtype=np.uint8).reshape(-1, 3))
        self._q_T.append(T.copy())
        if len(self._q_depth) >= self._batch:
            self.Flush()

    def Flush(self):
        if not self._q_depth:
            return
        warp = None
        if self.ctr_num_ > 0:
            warp = dict(ctr=self.grids_, resolution=self.ctr_resolution_, length=np.float32(self.ctr_length_),
                        grid_index=np.array(self._q_gi, np.int32), seg=np.array(self._q_seg), madj=np.array(self._q_madj))
        self.volume_.IntegrateFrames(np.stack(self._q_depth), np.array(self._q_T), warp)
        if self._q_color:
            if len(self._q_color) != len(self._q_depth):
                raise ValueError("IntegrateApp: %d of the %d queued frames carry colour" % (len(self._q_color), len(self._q_depth)))
            self.volume_.enable_color()
            self.volume_.ColorFrames(np.stack(self._q_depth), np.stack(self._q_color), np.array(self._q_T), warp)
        self.frames_integrated += len(self._q_depth)
        self._q_depth, self._q_T, self._q_gi, self._q_seg, self._q_madj = [], [], [], [], []
        self._q_color = []

    def Finish(self, save=True):
        self.Flush()
        if save:
            return self.volume_.SaveWorld(self.pcd_filename_)
        return None


def _inverse(T):
    """4x4 float64 inverse by cofactors -- same expansion as csrc/er_common.cpp so the host programs and
    this mirror hand identical matrices to the kernels."""
    m = np.asarray(T, np.float64).reshape(16)
    inv = np.empty(16, np.float64)
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10]
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10]
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9]
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9]
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10]
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10]
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9]
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9]
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6]
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6]
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5]
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5]
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6]
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6]
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5]
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5]
    det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12]
    det = 1.0 / det
    return (inv * det).reshape(4, 4)


def reproject_matrix(traj_f, traj_0, seg_0):
    """IntegrateApp.cpp:243: traj[f-1].inverse() * traj[0] * seg[0].inverse()."""
    return mat4_mul(mat4_mul(_inverse(traj_f), traj_0), _inverse(seg_0))

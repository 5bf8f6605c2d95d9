"""Fragments from a depth stream (include/er_hip.h er_frag_*, csrc/er_fragments.hip): every `interval` frames are tracked
frame-to-model against a TSDF volume of their own, `lanes` fragments in lockstep, and leave their frame poses and the oriented surface points
of that volume -- what pcl_kinfu_largeScale writes as 100-0.log and cloud_bin_<k>.pcd.  Every result is DepthOdometry.track_model's and
TSDFVolume.SaveFragment's, bit for bit, whatever the lane count.  There is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _ffi
from . import formats


def default_params():
    """er_frag_params_default as a dict (raycast = (t_min, t_max, step))."""
    p = _ffi.ErFragParams()
    _ffi.check(_ffi.lib().er_frag_params_default(C.byref(p)), "er_frag_params_default")
    return dict(interval=p.interval, lanes=p.lanes, max_units=p.max_units, length=np.float32(p.length),
                raycast=(np.float32(p.raycast.t_min), np.float32(p.raycast.t_max), np.float32(p.raycast.step)))


class FragmentBuilder:
    """er_frag_create(cols, rows, cam6 = fx fy cx cy ICP_trunc integration_trunc, or None for the reference's defaults).  odom_params: the
    fields of er_odom_params, as DepthOdometry takes them."""

    def __init__(self, cols, rows, cam6=None, interval=50, lanes=8, max_units=512, length=3.0, device=0, raycast=None, **odom_params):
        self._lib = _ffi.lib()
        op = _ffi.ErOdomParams()
        _ffi.check(self._lib.er_odom_params_default(C.byref(op)), "er_odom_params_default")
        for k, v in odom_params.items():
            if k == "iterations":
                it = list(v) + list(op.iterations)[len(v):]
                op.iterations = (C.c_int * 4)(*[int(x) for x in it[:4]])
            elif k in ("dist_thresh", "angle_thresh"):
                setattr(op, k, float(v))
            elif hasattr(op, k):
                setattr(op, k, int(v))
            else:
                raise TypeError("FragmentBuilder: unknown parameter %r" % k)
        fp = _ffi.ErFragParams()
        _ffi.check(self._lib.er_frag_params_default(C.byref(fp)), "er_frag_params_default")
        fp.interval, fp.lanes, fp.max_units, fp.length = int(interval), int(lanes), int(max_units), float(length)
        if raycast is not None:
            fp.raycast = _ffi.ErRaycastParams(*[float(np.float32(x)) for x in raycast])
        self.cols, self.rows, self.device = int(cols), int(rows), int(device)
        self.interval, self.lanes, self.max_units, self.length = int(interval), int(lanes), int(max_units), float(length)
        cam = None if cam6 is None else np.ascontiguousarray(cam6, dtype=np.float32).reshape(-1)
        if cam is not None and cam.size != 6:
            raise ValueError("cam6 = fx fy cx cy ICP_trunc integration_trunc")
        h = C.c_void_p()
        _ffi.check(self._lib.er_frag_create(self.cols, self.rows, None if cam is None else _ffi.ptr(cam), C.byref(op), C.byref(fp), self.device,
                                            C.byref(h)), "er_frag_create")
        self._h = h
        self.W = self.status = self.fragments = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.er_frag_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lane_bytes(self):
        """Device memory the first lane took when it was created."""
        b = C.c_size_t(0)
        _ffi.check(self._lib.er_frag_lane_bytes(self._h, C.byref(b)), "er_frag_lane_bytes")
        return b.value

    def build(self, depth, T0=None):
        """er_frag_build.  depth: uint16 millimetres [n, rows * cols], a numpy array or a torch tensor (one on the handle's device is read in
        place).  T0: None (the kinfu base pose), one 4 x 4 pose for every fragment's first frame, or one per fragment.  Returns
        (W [n, 4, 4] float64, status [n], [(xyz float32 [m, 3], normals float32 [m, 3]) per fragment])."""
        px = self.cols * self.rows
        keep = None
        if hasattr(depth, "data_ptr") and depth.is_cuda:
            import torch
            t = depth.contiguous()
            if t.element_size() != 2 or t.numel() % px:
                raise ValueError("depth tensor must hold 16-bit frames of %d x %d" % (self.cols, self.rows))
            if t.device.index is not None and t.device.index != self.device:
                raise ValueError("depth tensor lives on another device")
            torch.cuda.current_stream(t.device).synchronize()          # the frames must be complete before other streams read them
            keep, dp, on_dev, n = t, C.c_void_p(t.data_ptr()), 1, t.numel() // px
        else:
            if hasattr(depth, "data_ptr"):
                from . import synth
                depth = synth.to_numpy_u16(depth)
            keep = np.ascontiguousarray(depth, dtype=np.uint16).reshape(-1, px)
            dp, on_dev, n = _ffi.ptr(keep), 0, keep.shape[0]
        t0, n_t0 = None, 1
        if T0 is not None:
            t0 = np.ascontiguousarray(T0, np.float64).reshape(-1, 16)
            n_t0 = t0.shape[0]
        W = np.zeros((n, 4, 4), np.float64)
        status = np.zeros(n, np.int32)
        _ffi.check(self._lib.er_frag_build(self._h, n, dp, on_dev, None if t0 is None else _ffi.ptr(t0), n_t0, _ffi.ptr(W), _ffi.ptr(status)),
                   "er_frag_build")
        del keep
        k = C.c_int(0)
        _ffi.check(self._lib.er_frag_count(self._h, C.byref(k)), "er_frag_count")
        frags = []
        for f in range(k.value):
            m = C.c_long(0)
            _ffi.check(self._lib.er_frag_read(self._h, f, None, None, 0, C.byref(m)), "er_frag_read")
            xyz, nrm = np.empty((m.value, 3), np.float32), np.empty((m.value, 3), np.float32)
            if m.value:
                _ffi.check(self._lib.er_frag_read(self._h, f, _ffi.ptr(xyz), _ffi.ptr(nrm), m.value, C.byref(m)), "er_frag_read")
            frags.append((xyz, nrm))
        self.W, self.status, self.fragments = W, status, frags
        return W, status, frags

    def save(self, directory, seg_log=None):
        """The last build as files: <directory>/cloud_bin_<k>.pcd and the segment log (default <directory>/100-0.log), entry i = "i i i+1" and
        the pose of frame i in its fragment's frame.  Returns the paths written, the log last."""
        if self.W is None:
            raise ValueError("FragmentBuilder.save: nothing has been built")
        os.makedirs(directory, exist_ok=True)
        out = []
        for k, (xyz, nrm) in enumerate(self.fragments):
            out.append(os.path.join(directory, "cloud_bin_%d.pcd" % k))
            formats.save_pcd_xyzn(out[-1], xyz, nrm)
        seg_log = os.path.join(directory, "100-0.log") if seg_log is None else seg_log
        formats.save_log(seg_log, [formats.FramedTransformation(i, i, i + 1, T) for i, T in enumerate(self.W)])
        return out + [seg_log]

"""Depth odometry on the GPU (include/er_hip.h er_odom_*, csrc/er_odom.hip): KinFu-style projective point-to-plane ICP
between depth frames, batched over a pair list.  Frames are uint16 millimetres, numpy arrays or torch tensors that already live on the
handle's device (passed as a device pointer, as TSDFVolume.IntegrateFrames does).  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi

TRACE = 17          # ER_ODOM_TRACE
DEPTH_W_MAX = 512   # ER_ODOM_DEPTH_W


def default_params():
    """er_odom_params_default as a dict."""
    p = _ffi.ErOdomParams()
    _ffi.check(_ffi.lib().er_odom_params_default(C.byref(p)), "er_odom_params_default")
    return dict(levels=p.levels, iterations=tuple(p.iterations), bilateral=p.bilateral, max_depth_mm=p.max_depth_mm, min_valid=p.min_valid,
                dist_thresh=np.float32(p.dist_thresh), angle_thresh=np.float32(p.angle_thresh))


def tables():
    """er_odom_tables: (space float32 [73], depth_w float32 [n]) -- the weight tables of the bilateral filter as the kernels read them."""
    space, dw, n = np.zeros(73, np.float32), np.zeros(DEPTH_W_MAX, np.float32), C.c_int(0)
    _ffi.check(_ffi.lib().er_odom_tables(_ffi.ptr(space), _ffi.ptr(dw), C.byref(n)), "er_odom_tables")
    return space, dw[:n.value].copy()


def accumulate(T_rel, first=None):
    """world_T_camera [n + 1, 4, 4] from the relative poses T_rel[i] = frame i <- frame i + 1; every entry is
    ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in float64, the order bin/DepthOdometry uses."""
    W = [np.eye(4) if first is None else np.asarray(first, np.float64).reshape(4, 4).copy()]
    for T in np.asarray(T_rel, np.float64).reshape(-1, 4, 4):
        A, out = W[-1], np.empty((4, 4))
        for r in range(4):
            for c in range(4):
                out[r, c] = ((float(A[r, 0]) * float(T[0, c]) + float(A[r, 1]) * float(T[1, c])) + float(A[r, 2]) * float(T[2, c])) + float(A[r, 3]) * float(T[3, c])
        W.append(out)
    return np.stack(W)


class DepthOdometry:
    """er_odom_create(cols, rows, cam = (fx, fy, cx, cy), params).  Keyword parameters: the fields of er_odom_params."""

    def __init__(self, cols, rows, cam, device=0, **params):
        self._lib = _ffi.lib()
        p = _ffi.ErOdomParams()
        _ffi.check(self._lib.er_odom_params_default(C.byref(p)), "er_odom_params_default")
        for k, v in params.items():
            if k == "iterations":
                it = list(v) + list(p.iterations)[len(v):]
                p.iterations = (C.c_int * 4)(*[int(x) for x in it[:4]])
            elif k in ("dist_thresh", "angle_thresh"):
                setattr(p, k, float(v))
            elif hasattr(p, k):
                setattr(p, k, int(v))
            else:
                raise TypeError("DepthOdometry: unknown parameter %r" % k)
        self.cols, self.rows, self.device = int(cols), int(rows), int(device)
        self.cam = tuple(np.asarray(cam, np.float32).reshape(-1)[:4])
        cam4 = np.ascontiguousarray(np.asarray(cam, np.float32).reshape(-1)[:4])
        h = C.c_void_p()
        _ffi.check(self._lib.er_odom_create(self.cols, self.rows, cam4.ctypes.data_as(C.POINTER(C.c_float)), C.byref(p), self.device, C.byref(h)),
                   "er_odom_create")
        self._h = h
        self.levels = p.levels
        self.iterations = tuple(p.iterations)[:p.levels]
        self.total_iters = sum(self.iterations)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.er_odom_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _depth(self, depth, n_frames=None):
        """(keep-alive object, pointer, on_device, n_frames) of a stack of frames."""
        px = self.cols * self.rows
        if hasattr(depth, "data_ptr"):                       # a torch tensor
            t = depth.contiguous()
            if t.element_size() != 2 or t.numel() % px:
                raise ValueError("depth tensor must hold 16-bit frames of %d x %d" % (self.cols, self.rows))
            if t.is_cuda:
                if t.device.index is not None and t.device.index != self.device:
                    raise ValueError("depth tensor lives on another device")
                import torch
                torch.cuda.current_stream(t.device).synchronize()      # the frames must be complete before another stream reads them
                n = t.numel() // px
                if n_frames is not None and n != n_frames:
                    raise ValueError("expected %d frames, got %d" % (n_frames, n))
                return t, C.c_void_p(t.data_ptr()), 1, n
            from . import synth
            depth = synth.to_numpy_u16(t)
        a = np.ascontiguousarray(depth, dtype=np.uint16).reshape(-1, px)
        if n_frames is not None and a.shape[0] != n_frames:
            raise ValueError("expected %d frames, got %d" % (n_frames, a.shape[0]))
        return a, _ffi.ptr(a), 0, a.shape[0]

    def align_pairs(self, depth, model_idx, frame_idx, guess=None, window=0, trace=False, sums=False):
        """er_odom_align_pairs.  Returns (T [p, 4, 4] float64 m_T_c, status [p]) and, if asked for, trace [p, iterations, 17] and sums [p, 27]."""
        keep, dp, on_dev, n = self._depth(depth)
        mi = np.ascontiguousarray(model_idx, np.int32).reshape(-1)
        fi = np.ascontiguousarray(frame_idx, np.int32).reshape(-1)
        if mi.shape != fi.shape:
            raise ValueError("model_idx and frame_idx differ in length")
        m = mi.shape[0]
        g = None if guess is None else np.ascontiguousarray(guess, np.float64).reshape(m, 16)
        T = np.zeros((m, 4, 4), np.float64)
        status = np.zeros(m, np.int32)
        tr = np.zeros((m, self.total_iters, TRACE), np.float64) if trace else None
        sm = np.zeros((m, 27), np.float64) if sums else None
        _ffi.check(self._lib.er_odom_align_pairs(self._h, n, dp, on_dev, m, _ffi.ptr(mi), _ffi.ptr(fi), None if g is None else _ffi.ptr(g), _ffi.ptr(T),
                                                 _ffi.ptr(status), None if tr is None else _ffi.ptr(tr), None if sm is None else _ffi.ptr(sm), int(window)),
                   "er_odom_align_pairs")
        out = (T, status)
        if trace:
            out += (tr,)
        if sums:
            out += (sm,)
        return out

    def track(self, depth, window=0):
        """er_odom_track: (T_rel [n - 1, 4, 4] with T_rel[i] = frame i <- frame i + 1, status [n - 1])."""
        keep, dp, on_dev, n = self._depth(depth)
        T = np.zeros((max(n - 1, 0), 4, 4), np.float64)
        status = np.zeros(max(n - 1, 0), np.int32)
        _ffi.check(self._lib.er_odom_track(self._h, n, dp, on_dev, _ffi.ptr(T), _ffi.ptr(status), int(window)), "er_odom_track")
        return T, status

    def _model_records(self, model_maps):
        """(keep-alive tensors, void*[levels]) of a model: per level (depth, vertex map, normal map) as TSDFVolume.raycast returns them.  Device
        maps that are the two views of one record tensor are read in place; anything else is packed into records and uploaded."""
        import torch
        if len(model_maps) != self.levels:
            raise ValueError("the model has %d levels, the odometry %d" % (len(model_maps), self.levels))
        dev = torch.device("cuda", self.device)
        keep = []
        for l, (_, V, N) in enumerate(model_maps):
            c, r = self.cols >> l, self.rows >> l
            if tuple(V.shape) != (r, c, 3) or tuple(N.shape) != (r, c, 3):
                raise ValueError("level %d of the model is not %d x %d" % (l, c, r))
            in_place = (hasattr(V, "data_ptr") and V.is_cuda and V.device == dev and V.dtype == torch.float32 and N.dtype == torch.float32
                        and V.stride() == (8 * c, 8, 1) and N.stride() == (8 * c, 8, 1) and N.data_ptr() == V.data_ptr() + 16)
            if in_place:
                keep.append(V)
            else:
                rec = torch.zeros((r, c, 2, 4), dtype=torch.float32)
                rec[:, :, 0, :3] = torch.as_tensor(np.asarray(V.cpu() if hasattr(V, "cpu") else V, np.float32))
                rec[:, :, 1, :3] = torch.as_tensor(np.asarray(N.cpu() if hasattr(N, "cpu") else N, np.float32))
                keep.append(rec.to(dev))
        torch.cuda.current_stream(dev).synchronize()             # the records must be complete before another stream reads them
        return keep, (C.c_void_p * self.levels)(*[t.data_ptr() for t in keep])

    def align_model(self, model_maps, depth, guess=None, trace=False, sums=False, window=0):
        """er_frame_to_model_align: every frame of `depth` against ONE model, the per-level maps of TSDFVolume.raycast(T, cols, rows, cam,
        levels = self.levels) -- device = True is read in place.  Returns (T [n, 4, 4] float64 m_T_c = model <- frame, status [n]) and,
        if asked for, trace [n, iterations, 17] and sums [n, 27], like align_pairs."""
        keep_d, dp, on_dev, n = self._depth(depth)
        keep_m, recs = self._model_records(model_maps)
        g = None if guess is None else np.ascontiguousarray(guess, np.float64).reshape(n, 16)
        T = np.zeros((n, 4, 4), np.float64)
        status = np.zeros(n, np.int32)
        tr = np.zeros((n, self.total_iters, TRACE), np.float64) if trace else None
        sm = np.zeros((n, 27), np.float64) if sums else None
        _ffi.check(self._lib.er_frame_to_model_align(self._h, recs, n, dp, on_dev, None if g is None else _ffi.ptr(g), _ffi.ptr(T), _ffi.ptr(status),
                                                     None if tr is None else _ffi.ptr(tr), None if sm is None else _ffi.ptr(sm), int(window)),
                   "er_frame_to_model_align")
        del keep_d, keep_m
        out = (T, status)
        if trace:
            out += (tr,)
        if sums:
            out += (sm,)
        return out

    def align_models(self, models, depth, model_of_frame, guess=None, trace=False, sums=False, window=0):
        """er_frames_to_models_align: frame i of `depth` against models[model_of_frame[i]], each model what align_model takes.  Returns what
        align_model returns, and for every frame the bits of align_model(models[model_of_frame[i]], frame i)."""
        keep_d, dp, on_dev, n = self._depth(depth)
        keep_m, ptrs = [], []
        for m in models:
            k, r = self._model_records(m)
            keep_m.append(k)
            ptrs += list(r)
        recs = (C.c_void_p * len(ptrs))(*ptrs)
        mof = np.ascontiguousarray(model_of_frame, np.int32).reshape(-1)
        if mof.shape[0] != n:
            raise ValueError("model_of_frame names %d frames, depth holds %d" % (mof.shape[0], n))
        g = None if guess is None else np.ascontiguousarray(guess, np.float64).reshape(n, 16)
        T = np.zeros((n, 4, 4), np.float64)
        status = np.zeros(n, np.int32)
        tr = np.zeros((n, self.total_iters, TRACE), np.float64) if trace else None
        sm = np.zeros((n, 27), np.float64) if sums else None
        _ffi.check(self._lib.er_frames_to_models_align(self._h, len(models), recs, n, dp, on_dev, _ffi.ptr(mof), None if g is None else _ffi.ptr(g),
                                                       _ffi.ptr(T), _ffi.ptr(status), None if tr is None else _ffi.ptr(tr),
                                                       None if sm is None else _ffi.ptr(sm), int(window)), "er_frames_to_models_align")
        del keep_d, keep_m
        out = (T, status)
        if trace:
            out += (tr,)
        if sums:
            out += (sm,)
        return out

    def track_model(self, volume, depth, T0=None):
        """Frame-to-model tracking as a composition of public calls: frame 0 is integrated into `volume` (a TSDFVolume of the same image) at
        T0 (identity); every later frame is aligned against the volume ray-cast at the last pose, from the identity, T_i = T_{i-1} m_T_c,
        and integrated at T_i.  A lost frame keeps the last pose and is not integrated.  Returns (world_T_camera [n, 4, 4], status [n])."""
        from .tsdf import mat4_mul
        from . import synth
        frames = synth.to_numpy_u16(depth) if hasattr(depth, "data_ptr") else np.asarray(depth, np.uint16)
        frames = np.ascontiguousarray(frames).reshape(-1, self.rows * self.cols)
        n = frames.shape[0]
        W = np.zeros((n, 4, 4), np.float64)
        status = np.zeros(n, np.int32)
        if n == 0:
            return W, status
        W[0] = np.eye(4) if T0 is None else np.asarray(T0, np.float64).reshape(4, 4)
        volume.Integrate(frames[0], W[0])
        for i in range(1, n):
            model = volume.raycast(W[i - 1], self.cols, self.rows, self.cam, levels=self.levels, device=True)
            T, st = self.align_model(model, frames[i])
            status[i] = st[0]
            if st[0] != 0:
                W[i] = W[i - 1]
                continue
            W[i] = mat4_mul(W[i - 1], T[0])
            volume.Integrate(frames[i], W[i])
        return W, status

    def linearize(self, model, frame, level, T):
        """er_odom_linearize: (sums [27], count) at the pose T (m_T_c) on `level`."""
        if hasattr(model, "data_ptr"):
            import torch
            both = torch.stack([model.reshape(-1), frame.reshape(-1)])
        else:
            both = np.stack([np.asarray(model, np.uint16).reshape(-1), np.asarray(frame, np.uint16).reshape(-1)])
        keep, dp, on_dev, _ = self._depth(both, 2)
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        sums, count = np.zeros(27, np.float64), C.c_int(0)
        _ffi.check(self._lib.er_odom_linearize(self._h, dp, on_dev, int(level), _ffi.ptr(T), _ffi.ptr(sums), C.byref(count)), "er_odom_linearize")
        return sums, count.value

    def maps(self, frame, level):
        """er_odom_read_maps: (depth uint16 [r, c], vertex float32 [r, c, 3], normal float32 [r, c, 3]) of one frame on `level`."""
        keep, dp, on_dev, _ = self._depth(frame, 1)
        if not 0 <= int(level) < self.levels:
            raise _ffi.ErError("er_odom_read_maps failed: level = %d of %d" % (level, self.levels))
        c, r = self.cols >> level, self.rows >> level
        d, v, n = np.zeros((r, c), np.uint16), np.zeros((r, c, 3), np.float32), np.zeros((r, c, 3), np.float32)
        _ffi.check(self._lib.er_odom_read_maps(self._h, dp, on_dev, int(level), _ffi.ptr(d), _ffi.ptr(v), _ffi.ptr(n)), "er_odom_read_maps")
        return d, v, n

    tables = staticmethod(tables)

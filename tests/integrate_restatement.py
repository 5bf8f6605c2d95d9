"""numpy restatement of TSDFVolume::Integrate from ANY state (TSDFVolume.cpp:93-94), for volumes that do not start empty.

The oracle only starts from an empty volume, but it can supply a frame's inputs: one frame integrated alone into a fresh OracleVolume
leaves sdf_ = tsdf exactly ((0 * 0 + tsdf) / 1 is exact in float32) and weight_ = 1 on exactly the voxels the frame updates.  From a
given state the frame is then, on those voxels and in float32 as the reference has it,

    S = (S * W + tsdf) / (W + 1)
    W = W + 1

Every operation is an elementwise numpy float32 operation in the reference's order (w == 1: w * tsdf == tsdf).  A unit a frame touches
exists afterwards even where no voxel of it was updated, as in the reference.  tests/test_integrate_cases_cpu.py holds this to the
oracle's own sequential result from the empty state on every fixture."""
import numpy as np

from oracle.pyoracle import OracleVolume

UNIT_VOX = 64 ** 3
ONE = np.float32(1.0)


def frame_updates(depth, T, cols, rows, cam):
    """{key: (index array of the updated voxels, their float32 tsdf)} of one frame, and every unit key the frame touches."""
    ora = OracleVolume(cols, rows, cam)
    ora.Integrate(depth, T)
    out = {}
    for k in ora.unit_keys():
        sdf, w = ora.read_unit(int(k))
        idx = np.flatnonzero(w == ONE)
        assert idx.size == np.count_nonzero(w)
        out[int(k)] = (idx, sdf[idx].copy())
    ora.close()
    return out


class RestatedVolume:
    """unit_keys / read_unit / sum_weight like the volumes it is compared with."""

    def __init__(self, cols, rows, cam, state=None):
        self.cols, self.rows, self.cam = cols, rows, np.asarray(cam, np.float32)
        self.units = {}
        for k, (sdf, w) in (state or {}).items():
            self.units[int(k)] = (np.array(sdf, np.float32).reshape(-1), np.array(w, np.float32).reshape(-1))

    def Integrate(self, depth, T):
        for k, (idx, tsdf) in frame_updates(depth, T, self.cols, self.rows, self.cam).items():
            if k not in self.units:
                self.units[k] = (np.zeros(UNIT_VOX, np.float32), np.zeros(UNIT_VOX, np.float32))
            S, W = self.units[k]
            s, w = S[idx], W[idx]
            S[idx] = (s * w + tsdf) / (w + ONE)
            W[idx] = w + ONE
            assert S.dtype == np.float32 and W.dtype == np.float32

    def unit_keys(self):
        return np.array(sorted(self.units), np.int32)

    def read_unit(self, key):
        S, W = self.units[int(key)]
        return S.copy(), W.copy()

    def sum_weight(self):
        return float(sum(W.astype(np.float64).sum() for _, W in self.units.values()))

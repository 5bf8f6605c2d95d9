"""File formats of the ElasticReconstruction pipeline (the reference's real API).

Python mirror of the readers/writers the C++ host programs (csrc/host/er_formats.h) implement;
byte-compatible with the reference:

  .log   RGBDTrajectory::LoadFromFile / SaveToFile          Integrate/TSDFVolumeUnit.h:22-63, BuildCorrespondence/Helper.h:19-60
  .info  RGBDInformation::LoadFromFile / SaveToFile          BuildCorrespondence/Helper.h:74-119
  .ctr   ControlGrid::Load                                   Integrate/ControlGrid.cpp:15-34 (writer: FragmentOptimizer/OptApp.cpp:884-895)
  camera CameraParam::LoadFromFile                           Integrate/TSDFVolumeUnit.h:72-95
  corres_<i>_<j>.txt                                         BuildCorrespondence/CorresApp.cpp:175-184
  .pcd   binary / ascii PCD v0.7 (world.pcd: TSDFVolume.cpp:104-132; cloud_bin_<i>.pcd: CorresApp.cpp:88-90)
"""
import io
import os

import numpy as np


class FramedTransformation:
    """FramedTransformation (TSDFVolumeUnit.h:12-20): id1_, id2_, frame_, transformation_ (4x4 float64)."""

    __slots__ = ("id1", "id2", "frame", "T")

    def __init__(self, id1, id2, frame, T):
        self.id1, self.id2, self.frame = int(id1), int(id2), int(frame)
        self.T = np.asarray(T, dtype=np.float64).reshape(4, 4)


def _data_lines(path):
    with open(path, "r") as f:
        for line in f:
            yield line


def load_log(path):
    """RGBDTrajectory::LoadFromFile: records of 5 lines; a line whose first char is '#' is skipped only
    where a header is expected (TSDFVolumeUnit.h:34-49).  Missing file -> empty list (f == NULL)."""
    out = []
    if not os.path.exists(path):
        return out
    it = _data_lines(path)
    for line in it:
        if len(line) > 0 and line[0] != "#":
            hdr = line.split()
            try:
                ids = [int(float(x)) for x in hdr[:3]]
            except ValueError:
                continue
            if len(ids) < 3:
                continue
            rows = []
            for _ in range(4):
                r = next(it, None)
                if r is None:
                    break
                rows.append([float(x) for x in r.split()[:4]])
            if len(rows) < 4:
                break
            out.append(FramedTransformation(ids[0], ids[1], ids[2], np.array(rows, dtype=np.float64)))
    return out


def save_log(path, traj):
    """RGBDTrajectory::SaveToFile (TSDFVolumeUnit.h:52-62): "%d\\t%d\\t%d\\n" + 4 x "%.8f %.8f %.8f %.8f\\n"."""
    with open(path, "w") as f:
        for ft in traj:
            f.write("%d\t%d\t%d\n" % (ft.id1, ft.id2, ft.frame))
            for r in range(4):
                f.write("%.8f %.8f %.8f %.8f\n" % tuple(ft.T[r]))


class FramedInformation:
    """FramedInformation (Helper.h:64-72): id1_, id2_, frame_, information_ (row-major 6x6 float64)."""

    __slots__ = ("id1", "id2", "frame", "info")

    def __init__(self, id1, id2, frame, info):
        self.id1, self.id2, self.frame = int(id1), int(id2), int(frame)
        self.info = np.asarray(info, dtype=np.float64).reshape(6, 6)


def load_info(path):
    out = []
    if not os.path.exists(path):
        return out
    it = _data_lines(path)
    for line in it:
        if len(line) > 0 and line[0] != "#":
            hdr = line.split()
            if len(hdr) < 3:
                continue
            rows = []
            for _ in range(6):
                r = next(it, None)
                if r is None:
                    break
                rows.append([float(x) for x in r.split()[:6]])
            if len(rows) < 6:
                break
            out.append(FramedInformation(int(hdr[0]), int(hdr[1]), int(hdr[2]), np.array(rows)))
    return out


def save_info(path, infos):
    with open(path, "w") as f:
        for fi in infos:
            f.write("%d\t%d\t%d\n" % (fi.id1, fi.id2, fi.frame))
            for r in range(6):
                f.write("%.8f %.8f %.8f %.8f %.8f %.8f\n" % tuple(fi.info[r]))


def load_camera(path):
    """CameraParam::LoadFromFile (TSDFVolumeUnit.h:72-95): six floats, one per line.
    Returns float32[6] = fx fy cx cy ICP_trunc integration_trunc (defaults when the file is absent)."""
    cam = np.array([525.0, 525.0, 319.5, 239.5, 2.5, 2.5], dtype=np.float32)
    if path and os.path.exists(path):
        vals = []
        with open(path) as f:
            for line in f:
                if len(line) > 0 and line[0] != "#" and line.strip():
                    vals.append(np.float32(line.split()[0]))
        for i, v in enumerate(vals[:6]):
            cam[i] = v
    return cam


def save_camera(path, cam6):
    with open(path, "w") as f:
        for v in cam6:
            f.write("%.6f\n" % float(v))


def load_ctr(path, num, resolution):
    """ControlGrid::Load x num (IntegrateApp.cpp:49-55, ControlGrid.cpp:15-34): num * (res+1)^3 lines of
    "%f %f %f"; returns float32[num, (res+1)^3, 3]."""
    verts = (resolution + 1) ** 3
    out = np.zeros((num, verts, 3), dtype=np.float32)
    with open(path) as f:
        for g in range(num):
            for i in range(verts):
                line = f.readline()
                if not line:
                    return out
                if line[0] != "#":
                    p = line.split()
                    out[g, i] = [np.float32(p[0]), np.float32(p[1]), np.float32(p[2])]
    return out


def save_ctr(path, grids):
    """Writer matching FragmentOptimizer/OptApp.cpp:884-895: "%.10f %.10f %.10f\\n" per vertex."""
    g = np.asarray(grids, dtype=np.float64).reshape(-1, 3)
    with open(path, "w") as f:
        for v in g:
            f.write("%.10f %.10f %.10f\n" % (v[0], v[1], v[2]))


def save_corres(path, pairs):
    """corres_<i>_<j>.txt (CorresApp.cpp:178-183): "%d %d\\n" = index in fragment i, index in fragment j."""
    with open(path, "w") as f:
        for a, b in np.asarray(pairs).reshape(-1, 2):
            f.write("%d %d\n" % (a, b))


def load_corres(path):
    if os.path.getsize(path) == 0:
        return np.zeros((0, 2), dtype=np.int32)
    return np.loadtxt(path, dtype=np.int32).reshape(-1, 2)


# ---------------------------------------------------------------------------------- PCD v0.7
_PCD_NP = {("F", 4): np.float32, ("F", 8): np.float64, ("U", 1): np.uint8, ("U", 2): np.uint16, ("U", 4): np.uint32,
           ("I", 1): np.int8, ("I", 2): np.int16, ("I", 4): np.int32}


def lzf_decompress(src, out_len):
    """LZF decoder (format per Matlab_Toolbox/External/matpcl/lzfd.m:21-76)."""
    src = memoryview(src)
    out = bytearray(out_len)
    ip, op, n = 0, 0, len(src)
    while ip < n:
        ctrl = src[ip]
        ip += 1
        if ctrl < 32:
            ln = ctrl + 1
            out[op:op + ln] = src[ip:ip + ln]
            ip += ln
            op += ln
        else:
            ln = ctrl >> 5
            if ln == 7:
                ln += src[ip]
                ip += 1
            ref = op - ((ctrl & 0x1F) << 8) - src[ip] - 1
            ip += 1
            for _ in range(ln + 2):
                out[op] = out[ref]
                op += 1
                ref += 1
    return bytes(out[:op])


def lzf_compress(data):
    """LZF encoder (the stream lzf_decompress / PCL's binary_compressed reader take): greedy matcher over a hash of 3-byte
    strings, back references of 3..264 bytes up to 8192 bytes back, literal runs of up to 32 bytes.  Pure Python -- meant
    for the sample-sized clouds this package writes, the C++ programs have their own (csrc/host/er_formats.h)."""
    src = bytes(data)
    n = len(src)
    out = bytearray()
    last = {}
    lit = 0
    i = 0

    def flush(end):
        nonlocal lit
        while lit < end:
            run = min(32, end - lit)
            out.append(run - 1)
            out.extend(src[lit:lit + run])
            lit += run

    while i + 2 < n:
        key = src[i:i + 3]
        ref = last.get(key, -1)
        last[key] = i
        if ref >= 0 and i - ref <= 8192:
            cap = min(n - i, 264)
            ln = 3
            while ln < cap and src[ref + ln] == src[i + ln]:
                ln += 1
            flush(i)
            back, l = i - ref - 1, ln - 2
            if l < 7:
                out.append((l << 5) | (back >> 8))
            else:
                out.append((7 << 5) | (back >> 8))
                out.append(l - 7)
            out.append(back & 0xFF)
            for k in range(i + 1, min(i + ln, n - 2)):
                last[src[k:k + 3]] = k
            i += ln
            lit = i
        else:
            i += 1
    flush(n)
    return bytes(out)


def save_pcd_compressed(path, fields):
    """pcl::PCDWriter::writeBinaryCompressed layout (FragmentOptimizer's sample.pcd, OptApp.cpp:921-922): `fields` is an
    ordered mapping name -> float32 column; columns are stored one after another, LZF-compressed, behind the two sizes."""
    names = list(fields)
    cols = [np.ascontiguousarray(fields[k], np.float32).reshape(-1) for k in names]
    n = cols[0].shape[0] if cols else 0
    assert all(c.shape[0] == n for c in cols)
    raw = b"".join(c.tobytes() for c in cols)
    packed = lzf_compress(raw)
    k = len(names)
    with open(path, "wb") as f:
        f.write(("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\nCOUNT %s\nWIDTH %d\nHEIGHT 1\n"
                 "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary_compressed\n"
                 % (" ".join(names), " ".join(["4"] * k), " ".join(["F"] * k), " ".join(["1"] * k), n, n)).encode("ascii"))
        f.write(np.array([len(packed), len(raw)], np.uint32).tobytes())
        f.write(packed)


def load_pcd(path):
    """Reads ascii / binary / binary_compressed PCD v0.7 with an arbitrary field list
    (format per Matlab_Toolbox/External/matpcl/loadpcd.m:33-224).  Returns dict field -> 1-D array."""
    with open(path, "rb") as f:
        raw = f.read()
    hdr = {}
    pos = 0
    while True:
        end = raw.index(b"\n", pos)
        line = raw[pos:end].decode("ascii", "replace").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        k, _, v = line.partition(" ")
        hdr[k.upper()] = v.split()
        if k.upper() == "DATA":
            break
    fields = hdr["FIELDS"]
    sizes = [int(x) for x in hdr["SIZE"]]
    types = hdr["TYPE"]
    counts = [int(x) for x in hdr.get("COUNT", ["1"] * len(fields))]
    npts = int(hdr["POINTS"][0]) if "POINTS" in hdr else int(hdr["WIDTH"][0]) * int(hdr["HEIGHT"][0])
    mode = hdr["DATA"][0]
    dts = [np.dtype(_PCD_NP[(t, s)]) for t, s in zip(types, sizes)]
    out = {}
    if mode == "ascii":
        txt = raw[pos:].decode("ascii", "replace").split()
        ncol = sum(counts)
        arr = np.array(txt[:npts * ncol]).reshape(npts, ncol)
        c = 0
        for name, dt, cnt in zip(fields, dts, counts):
            col = arr[:, c:c + cnt]
            out[name] = (col.astype(np.float64).astype(dt) if dt.kind != "f" else col.astype(dt)).reshape(npts, cnt).squeeze(-1) if cnt == 1 else col.astype(dt)
            c += cnt
        return out
    if mode == "binary":
        rec = np.dtype([(name if name != "_" else "_pad%d" % i, dt, (cnt,)) if cnt > 1 else (name if name != "_" else "_pad%d" % i, dt)
                        for i, (name, dt, cnt) in enumerate(zip(fields, dts, counts))])
        a = np.frombuffer(raw, dtype=rec, count=npts, offset=pos)
        for name in a.dtype.names:
            if not name.startswith("_pad"):
                out[name] = np.ascontiguousarray(a[name])
        return out
    if mode == "binary_compressed":
        csz, usz = np.frombuffer(raw, dtype=np.uint32, count=2, offset=pos)
        blob = lzf_decompress(raw[pos + 8:pos + 8 + int(csz)], int(usz))
        off = 0
        for name, dt, cnt in zip(fields, dts, counts):   # field-major (SoA) after decompression
            nb = dt.itemsize * cnt * npts
            if name != "_":
                a = np.frombuffer(blob, dtype=dt, count=npts * cnt, offset=off)
                out[name] = a.reshape(npts, cnt).squeeze(-1) if cnt == 1 else a.reshape(npts, cnt)
            off += nb
        return out
    raise ValueError("unsupported PCD DATA mode %r" % mode)


def save_pcd_xyzi(path, xyzi):
    """world.pcd exactly as pcl::io::savePCDFile( name, PointCloud<PointXYZI>, binary=true ) lays it out
    (TSDFVolume.cpp:130): FIELDS x y z intensity, float32, DATA binary."""
    a = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
    n = a.shape[0]
    with open(path, "wb") as f:
        f.write(("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\n"
                 "TYPE F F F F\nCOUNT 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n"
                 % (n, n)).encode("ascii"))
        f.write(a.tobytes())


def save_pcd_xyzn(path, xyz, normals, binary=True):
    """cloud_bin_<i>.pcd-style fragment: FIELDS x y z normal_x normal_y normal_z (float32)."""
    a = np.concatenate([np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(normals, np.float32).reshape(-1, 3)], axis=1)
    n = a.shape[0]
    with open(path, "wb") as f:
        f.write(("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z normal_x normal_y normal_z\n"
                 "SIZE 4 4 4 4 4 4\nTYPE F F F F F F\nCOUNT 1 1 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\n"
                 "POINTS %d\nDATA %s\n" % (n, n, "binary" if binary else "ascii")).encode("ascii"))
        if binary:
            f.write(np.ascontiguousarray(a).tobytes())
        else:
            s = io.StringIO()
            np.savetxt(s, a, fmt="%.9g")
            f.write(s.getvalue().encode("ascii"))


def _ply_header(n, m, normals, binary, colors=False):
    return ("ply\nformat %s 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s%s"
            "element face %d\nproperty list uchar int vertex_indices\nend_header\n"
            % ("binary_little_endian" if binary else "ascii", n,
               "property float nx\nproperty float ny\nproperty float nz\n" if normals else "",
               "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n" if colors else "", m))


def save_ply(path, verts, tris, normals=None, binary=True, colors=None):
    """A triangle mesh as PLY (what kinfu's mesh output leaves for a viewer; csrc/host/er_formats.h's save_ply writes the same bytes).
    verts: float32[n, 3] -- or [n, 4], TSDFVolume.extract_indexed_mesh's x y z axis rows: the fourth column is not written; tris: int32[m, 3];
    normals: float32[n, 3] or None.  A normal with a NaN component is written as 0 0 0: the ABI keeps the NaN ("no normal"), a viewer chokes
    on it, and a zero vector is what mesh tools take for "unset".  colors: uint8[n, 4] = red green blue alpha (TSDFVolume.sample_colors) or None,
    written as four uchar properties behind the normals.  binary: little-endian float32 / uchar 3 + int32 rows, a vertex row with colours the
    packed floats followed by its four bytes; ascii: %.9g floats, the colours as integers, one space between columns.  With colors = None the
    file is byte for byte what it was before colour existed."""
    v = np.asarray(verts, np.float32)
    if v.ndim != 2 or v.shape[1] not in (3, 4):
        raise ValueError("save_ply: verts must be [n, 3] or [n, 4], not %s" % (v.shape,))
    v = np.ascontiguousarray(v[:, :3])
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    cols = [v]
    if normals is not None:
        nr = np.array(normals, np.float32).reshape(-1, 3)
        if nr.shape[0] != v.shape[0]:
            raise ValueError("save_ply: %d normals for %d vertices" % (nr.shape[0], v.shape[0]))
        nr[np.isnan(nr).any(axis=1)] = 0.0
        cols.append(nr)
    a = np.ascontiguousarray(np.concatenate(cols, axis=1))
    c = None
    if colors is not None:
        c = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 4)
        if c.shape[0] != v.shape[0]:
            raise ValueError("save_ply: %d colours for %d vertices" % (c.shape[0], v.shape[0]))
    with open(path, "wb") as f:
        f.write(_ply_header(v.shape[0], t.shape[0], normals is not None, binary, c is not None).encode("ascii"))
        if binary:
            if c is None:
                f.write(a.astype("<f4").tobytes())
            else:
                row = np.empty(v.shape[0], np.dtype([("f", "<f4", (a.shape[1],)), ("c", "u1", (4,))]))
                row["f"] = a
                row["c"] = c
                f.write(row.tobytes())
            face = np.empty(t.shape[0], np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
            face["n"] = 3
            face["i"] = t
            f.write(face.tobytes())
        else:
            s = io.StringIO()
            if c is None:
                np.savetxt(s, a, fmt="%.9g")
            else:
                np.savetxt(s, np.concatenate([a.astype(np.float64), c.astype(np.float64)], axis=1), fmt=["%.9g"] * a.shape[1] + ["%d"] * 4)
            np.savetxt(s, np.concatenate([np.full((t.shape[0], 1), 3, np.int32), t], axis=1), fmt="%d")
            f.write(s.getvalue().encode("ascii"))


_PLY_COLOR_PROPS = ["red", "green", "blue", "alpha"]


def _load_ply(path):
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    if lines[0] != "ply":
        raise ValueError("%s is not a PLY file" % path)
    mode, n, m, props, types, cur = None, 0, 0, [], [], None
    for line in lines[1:]:
        w = line.split()
        if not w or w[0] == "comment":
            continue
        if w[0] == "format":
            mode = w[1]
        elif w[0] == "element":
            cur = w[1]
            if cur == "vertex":
                n = int(w[2])
            elif cur == "face":
                m = int(w[2])
        elif w[0] == "property" and cur == "vertex":
            if w[1] != ("uchar" if w[2] in _PLY_COLOR_PROPS else "float"):
                raise ValueError("load_ply: vertex property %s is not a %s" % (w[-1], "uchar" if w[2] in _PLY_COLOR_PROPS else "float"))
            props.append(w[2])
        elif w[0] == "property" and cur == "face" and w[1:4] != ["list", "uchar", "int"]:
            raise ValueError("load_ply: faces must be 'list uchar int'")
    has_c = props[-4:] == _PLY_COLOR_PROPS
    fprops = props[:-4] if has_c else props
    if fprops not in (["x", "y", "z"], ["x", "y", "z", "nx", "ny", "nz"]):
        raise ValueError("load_ply: vertex properties %s" % props)
    k = len(fprops)
    c = None
    if mode == "binary_little_endian":
        if has_c:
            row = np.frombuffer(raw, np.dtype([("f", "<f4", (k,)), ("c", "u1", (4,))]), n, end)
            a, c, vbytes = row["f"].astype(np.float32).reshape(n, k), np.ascontiguousarray(row["c"]).reshape(n, 4), (4 * k + 4) * n
        else:
            a, vbytes = np.frombuffer(raw, "<f4", n * k, end).reshape(n, k).astype(np.float32), 4 * n * k
        face = np.frombuffer(raw, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), m, end + vbytes)
        if m and (face["n"] != 3).any():
            raise ValueError("load_ply: a face is not a triangle")
        t = face["i"].astype(np.int32).reshape(m, 3)
    elif mode == "ascii":
        tok = raw[end:].decode("ascii").split()
        kk = k + (4 if has_c else 0)
        rows = np.array(tok[:n * kk], dtype=object).reshape(n, kk)
        a = rows[:, :k].astype(np.float32).reshape(n, k)
        if has_c:
            c = rows[:, k:].astype(np.int64).astype(np.uint8).reshape(n, 4)
        ft = np.array(tok[n * kk:n * kk + 4 * m], dtype=np.int64).reshape(m, 4)
        if m and (ft[:, 0] != 3).any():
            raise ValueError("load_ply: a face is not a triangle")
        t = ft[:, 1:].astype(np.int32)
    else:
        raise ValueError("load_ply: unsupported format %r" % mode)
    return np.ascontiguousarray(a[:, :3]), np.ascontiguousarray(t), (np.ascontiguousarray(a[:, 3:]) if k == 6 else None), c


def load_ply(path):
    """Reads what save_ply writes (and any PLY of that shape: float x y z, optionally nx ny nz, optionally uchar red green blue alpha, faces as
    list uchar int, triangles only).  Returns (verts float32[n, 3], tris int32[m, 3], normals float32[n, 3] or None); the colours of a coloured
    file come from load_ply_colors."""
    return _load_ply(path)[:3]


def load_ply_colors(path):
    """load_ply with the per-vertex colours: (verts, tris, normals or None, colors uint8[n, 4] or None)."""
    return _load_ply(path)


# GlobalRegistration's alignment.config (helper.h's Configuration): key=value lines.  The defaults are the values of the file the reference ships.
ALIGNMENT_DEFAULTS = dict(visualization=False, estimate_normal=True, aux_data=False, smart_swap=True, pcl_verbose=3, normal_radius=0.1,
                          feature_radius=0.25, max_iteration=4000000, num_of_samples=4, correspondence_randomness=2, edge_similarity=0.9,
                          resample_leaf=0.05, max_correspondence_distance=0.075, inlier_fraction=0.33, inlier_number=30000,
                          angle_difference=0.52359878)


def load_alignment_config(path):
    """alignment.config -> dict.  Known keys are converted to the type of their default (booleans: "true" is True, anything else False,
    as the reference compares); unknown keys are kept as strings; path None or a missing file gives the defaults."""
    cfg = dict(ALIGNMENT_DEFAULTS)
    if path is None or not os.path.exists(path):
        return cfg
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or "=" not in line:
                continue
            key, val = line.split("=", 1)
            key, val = key.strip(), val.strip()
            d = ALIGNMENT_DEFAULTS.get(key)
            if isinstance(d, bool):
                cfg[key] = val == "true"
            elif isinstance(d, int):
                cfg[key] = int(val)
            elif isinstance(d, float):
                cfg[key] = float(val)
            else:
                cfg[key] = val
    return cfg

// er_fragments.hip -- the fragment builder of liber_hip.so: a depth stream in, per fragment the frame poses and the oriented
// surface points of its TSDF volume out -- the step pcl_kinfu_largeScale does in the real pipeline (the reference tree does not contain it).
// Host code only: the kernels are the ray caster's (er_tsdf_raycast.hip: k_raycast_batch), the odometry's (er_odom.hip) and path A's.
//
// Frame-to-model tracking is sequential inside a fragment and independent between fragments, so `lanes` fragments run in LOCKSTEP: per step one
// ray-cast launch over lanes x levels jobs, one alignment run with one pair per lane, one single-frame integration per lane.  What a lane
// computes is DepthOdometry.track_model on its fragment's frames, call for call (the same kernels on the same data in the same order per
// volume), so every pose, status, point and normal is the same bits whatever the lane count and whichever lane a fragment lands on.
#include "er_common.h"
#include "er_mem.h"

#include "../../include/er_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace {

struct Lane {
  er_tsdf_t vol = nullptr;
  er::DevScope mem;              // owns rec[]
  std::vector<void*> rec;        // [levels] record maps of the lane's model, device memory
  int frag = -1;                 // the fragment in flight (-1: idle)
  int pos = 0;                   // its next frame, counted from the fragment's first
  double W[16];                  // pose of the last frame
};

struct Fragment {
  std::vector<float> xyz, nrm;   // [m][3] each
};

}  // namespace

struct er_frag_s {
  int device = 0, cols = 0, rows = 0, levels = 0;
  float cam4[4];
  er_frag_params P{};
  er_odom_t odom = nullptr;
  std::vector<Lane> lanes;
  std::vector<Fragment> frags;
  size_t lane_bytes = 0;         // device memory one lane took (measured on the first)
};

namespace {

void frag_free(er_frag_s* h) {
  (void)hipSetDevice(h->device);
  for (Lane& L : h->lanes) {
    if (L.vol) er_tsdf_destroy(L.vol);
    L.mem.free_all();
  }
  if (h->odom) er_odom_destroy(h->odom);
  delete h;
}

// What a lane is expected to take: the unit pool and the batch staging of its volume (er_tsdf_create), and its record maps.
size_t lane_estimate(int cols, int rows, int max_units, int levels) {
  const size_t px = (size_t)cols * rows;
  size_t rec = 0;
  for (int l = 0; l < levels; l++) rec += (px >> (2 * l)) * 32;
  return (size_t)max_units * ER_UNIT_VOX * 8 + px * ER_MAX_BATCH * (3 * 4 + 3 * 2 + 3 * 2 * 4) + rec;
}

// The lane's fragment is complete: its oriented points inside the cube, NaN-normal rows kept (TSDFVolume.SaveFragment), then an empty volume.
int finish_fragment(er_frag_s* h, Lane& L) {
  long n = 0;
  if (er_tsdf_extract_oriented(L.vol, nullptr, nullptr, 0, &n)) return 1;
  std::vector<float> pts((size_t)n * 4), nrm((size_t)n * 4);
  if (n > 0 && er_tsdf_extract_oriented(L.vol, pts.data(), nrm.data(), n, &n)) return 1;
  Fragment& F = h->frags[(size_t)L.frag];
  const float len = h->P.length;
  for (long i = 0; i < n; i++) {
    const float* p = &pts[(size_t)i * 4];
    if (p[0] >= 0.0f && p[0] < len && p[1] >= 0.0f && p[1] < len && p[2] >= 0.0f && p[2] < len) {
      F.xyz.insert(F.xyz.end(), p, p + 3);
      F.nrm.insert(F.nrm.end(), &nrm[(size_t)i * 4], &nrm[(size_t)i * 4] + 3);
    }
  }
  return er_tsdf_reset(L.vol);
}

}  // namespace

extern "C" {

int er_frag_params_default(er_frag_params* p) {
  if (!p) return er::fail("er_frag_params_default: NULL argument");
  p->interval = 50;
  p->lanes = 8;
  p->max_units = 512;
  p->length = 3.0f;
  return er_raycast_params_default(&p->raycast);
}

int er_frag_create(int cols, int rows, const float cam6[6], const er_odom_params* odom_params, const er_frag_params* frag_params, int device,
                   er_frag_t* out) {
  const char* who = "er_frag_create";
  if (!out) return er::fail("%s: out is NULL", who);
  *out = nullptr;
  er_frag_params P;
  er_frag_params_default(&P);
  if (frag_params) P = *frag_params;
  if (P.interval < 1) return er::fail("%s: interval = %d, must be at least 1", who, P.interval);
  if (P.lanes < 1 || P.lanes > 64) return er::fail("%s: lanes = %d, must be 1 .. 64", who, P.lanes);
  if (P.max_units < 1) return er::fail("%s: max_units = %d, must be positive", who, P.max_units);
  if (!(P.length > 0.0f) || !std::isfinite(P.length)) return er::fail("%s: length must be positive and finite", who);
  if (er_device_count() <= 0) return er::fail("%s: no HIP device available (liber_hip has no CPU fallback)", who);
  er_frag_s* h = new er_frag_s;
  h->device = device;
  h->cols = cols;
  h->rows = rows;
  h->P = P;
  const float def[4] = {525.0f, 525.0f, 319.5f, 239.5f};               // er_tsdf_create's defaults
  for (int q = 0; q < 4; q++) h->cam4[q] = cam6 ? cam6[q] : def[q];
  if (er_odom_create(cols, rows, h->cam4, odom_params, device, &h->odom)) {
    frag_free(h);
    return 1;
  }
  h->levels = er::odom_levels(h->odom);
  h->lanes.resize((size_t)P.lanes);
  const size_t estimate = lane_estimate(cols, rows, P.max_units, h->levels);
  for (int k = 0; k < P.lanes; k++) {
    Lane& L = h->lanes[(size_t)k];
    size_t free0 = 0, free1 = 0, total = 0;
    (void)hipMemGetInfo(&free0, &total);
    bool ok = er_tsdf_create(cols, rows, cam6, P.max_units, device, &L.vol) == 0;
    L.rec.assign((size_t)h->levels, nullptr);
    for (int l = 0; ok && l < h->levels; l++)
      ok = L.mem.alloc(&L.rec[(size_t)l], (size_t)(cols >> l) * (rows >> l) * 32, who) == 0;
    if (!ok) {
      const size_t need = h->lane_bytes ? h->lane_bytes : estimate;
      std::string why = er_last_error();
      frag_free(h);
      return er::fail("%s: lane %d of %d cannot be allocated: a lane takes %zu bytes of device memory, %zu are free (%s)", who, k, P.lanes, need, free0,
                      why.c_str());
    }
    (void)hipMemGetInfo(&free1, &total);
    if (k == 0 && free0 > free1) h->lane_bytes = free0 - free1;
  }
  *out = h;
  return 0;
}

int er_frag_destroy(er_frag_t h) {
  if (!h) return 0;
  frag_free(h);
  return 0;
}

int er_frag_lane_bytes(er_frag_t h, size_t* bytes) {
  if (!h || !bytes) return er::fail("er_frag_lane_bytes: NULL argument");
  *bytes = h->lane_bytes;
  return 0;
}

int er_frag_build(er_frag_t h, int n_frames, const uint16_t* depth, int depth_on_device, const double* T0, int n_T0, double* W_out, int* status) {
  const char* who = "er_frag_build";
  if (!h) return er::fail("%s: NULL handle", who);
  if (n_frames < 0) return er::fail("%s: n_frames = %d is negative", who, n_frames);
  const int interval = h->P.interval;
  const int n_frag = (n_frames + interval - 1) / interval;
  if (T0 && n_T0 != 1 && n_T0 != n_frag) return er::fail("%s: n_T0 = %d, must be 1 or the fragment count %d", who, n_T0, n_frag);
  h->frags.assign((size_t)n_frag, Fragment());
  if (n_frames == 0) return 0;
  if (!depth || !W_out || !status) return er::fail("%s: NULL argument", who);
  ER_HIP_TRY(hipSetDevice(h->device));
  const size_t px = (size_t)h->cols * h->rows;
  // Host depth is uploaded once; the odometry and the lane volumes read that copy.
  er::DevScope own;
  uint16_t* d_own = nullptr;
  if (!depth_on_device) {
    const size_t bytes = (size_t)n_frames * px * sizeof(uint16_t);
    if (own.alloc(&d_own, (size_t)n_frames * px, who)) return 1;
    const hipError_t e = hipMemcpy(d_own, depth, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      return er::fail("%s: %zu bytes for the depth stream on the device: %s", who, bytes, hipGetErrorString(e));
    }
  }
  const uint16_t* d_depth = depth_on_device ? depth : d_own;
  double base[16];
  er::frag_basepose((double)h->P.length, base);
  const int levels = h->levels, n_lanes = (int)h->lanes.size();
  for (Lane& L : h->lanes) L.frag = -1;
  int next_frag = 0, rc = 0;
  auto take = [&](Lane& L) {                                            // the lane's next fragment, if one is left
    L.frag = next_frag < n_frag ? next_frag++ : -1;
    L.pos = 0;
  };
  for (Lane& L : h->lanes) {
    if (er_tsdf_reset(L.vol)) rc = 1;                                   // (whatever a failed call left)
    take(L);
  }
  // per step: the lanes that track (pos > 0), in lane order
  std::vector<int> who_tracks, cols, rows, mi, fi, st;
  std::vector<er_tsdf_t> vols;
  std::vector<float> cam;
  std::vector<double> poses, Tm;
  std::vector<er_raycast_params> rp;
  std::vector<void*> recs;
  std::vector<uint16_t*> no_depth;
  while (!rc) {
    who_tracks.clear();
    bool any = false;
    for (int k = 0; k < n_lanes; k++) {
      Lane& L = h->lanes[(size_t)k];
      if (L.frag < 0) continue;
      any = true;
      const int frame = L.frag * interval + L.pos;
      if (L.pos == 0) {                                                 // the fragment's first frame: integrated at T0, never lost
        const double* t0 = !T0 ? base : T0 + (n_T0 == 1 ? 0 : (size_t)L.frag * 16);
        std::copy(t0, t0 + 16, L.W);
        std::copy(t0, t0 + 16, W_out + (size_t)frame * 16);
        status[frame] = ER_ODOM_OK;
        if (er_tsdf_integrate_frames(L.vol, 1, d_depth + (size_t)frame * px, 1, L.W, nullptr)) rc = 1;
      } else {
        who_tracks.push_back(k);
      }
    }
    if (!any || rc) break;
    const int m = (int)who_tracks.size();
    if (m > 0) {
      // (1) every tracking lane's volume ray-cast at its last pose, all levels, in ONE launch.  er_tsdf_raycast_batch stands behind each
      //     volume's queued integration and returns when the records are complete.
      vols.clear(), cols.clear(), rows.clear(), cam.clear(), poses.clear(), rp.clear(), recs.clear();
      for (int k : who_tracks) {
        Lane& L = h->lanes[(size_t)k];
        for (int l = 0; l < levels; l++) {
          vols.push_back(L.vol);
          cols.push_back(h->cols >> l);
          rows.push_back(h->rows >> l);
          for (int q = 0; q < 4; q++) cam.push_back(h->cam4[q] / (float)(1 << l));
          poses.insert(poses.end(), L.W, L.W + 16);
          rp.push_back(h->P.raycast);
          recs.push_back(L.rec[(size_t)l]);
        }
      }
      no_depth.assign(recs.size(), nullptr);
      if (er_tsdf_raycast_batch((int)vols.size(), vols.data(), cols.data(), rows.data(), cam.data(), poses.data(), rp.data(), recs.data(), no_depth.data())) {
        rc = 1;
        break;
      }
      // (2) one alignment run: lane q's frame against model q, from the identity.  Returns when the states are on the host.
      mi.resize((size_t)m), fi.resize((size_t)m), st.resize((size_t)m), Tm.resize((size_t)m * 16);
      for (int q = 0; q < m; q++) {
        const Lane& L = h->lanes[(size_t)who_tracks[(size_t)q]];
        mi[(size_t)q] = n_frames + q;
        fi[(size_t)q] = L.frag * interval + L.pos;
      }
      if (er::odom_align_models(h->odom, who, m, recs.data(), n_frames, d_depth, 1, m, mi.data(), fi.data(), nullptr, Tm.data(), st.data(), nullptr, nullptr,
                                2 * n_lanes)) {
        rc = 1;
        break;
      }
      // (3) W_i = W_{i-1} m_T_c, and the frame into the lane's volume (asynchronous) unless it was lost
      for (int q = 0; q < m && !rc; q++) {
        Lane& L = h->lanes[(size_t)who_tracks[(size_t)q]];
        const int frame = fi[(size_t)q];
        status[frame] = st[(size_t)q];
        if (st[(size_t)q] == ER_ODOM_OK) {
          er::mat4_mul(L.W, &Tm[(size_t)q * 16], L.W);
          if (er_tsdf_integrate_frames(L.vol, 1, d_depth + (size_t)frame * px, 1, L.W, nullptr)) rc = 1;
        }
        std::copy(L.W, L.W + 16, W_out + (size_t)frame * 16);
      }
    }
    // (4) a lane behind its fragment's last frame hands the fragment over and takes the next one
    for (int k = 0; k < n_lanes && !rc; k++) {
      Lane& L = h->lanes[(size_t)k];
      if (L.frag < 0) continue;
      L.pos++;
      if (L.frag * interval + L.pos >= std::min((L.frag + 1) * interval, n_frames)) {
        if (finish_fragment(h, L)) rc = 1;
        take(L);
      }
    }
  }
  if (rc) {                                                             // nothing of a failed call may still read the depth copy
    std::string why = er_last_error();
    for (Lane& L : h->lanes) (void)er_tsdf_synchronize(L.vol);
    er::fail("%s", why.c_str());
  }
  return rc;
}

int er_frag_count(er_frag_t h, int* n_fragments) {
  if (!h || !n_fragments) return er::fail("er_frag_count: NULL argument");
  *n_fragments = (int)h->frags.size();
  return 0;
}

int er_frag_read(er_frag_t h, int fragment, float* xyz_out, float* normals_out, long capacity, long* count) {
  if (!h || !count) return er::fail("er_frag_read: NULL argument");
  if (fragment < 0 || fragment >= (int)h->frags.size()) return er::fail("er_frag_read: fragment %d of %d", fragment, (int)h->frags.size());
  const Fragment& F = h->frags[(size_t)fragment];
  *count = (long)(F.xyz.size() / 3);
  if (!xyz_out && !normals_out) return 0;
  if (capacity < *count) return er::fail("er_frag_read: capacity %ld < %ld points", capacity, *count);
  if (xyz_out) std::copy(F.xyz.begin(), F.xyz.end(), xyz_out);
  if (normals_out) std::copy(F.nrm.begin(), F.nrm.end(), normals_out);
  return 0;
}

}  // extern "C"

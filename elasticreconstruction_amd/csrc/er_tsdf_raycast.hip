// er_tsdf_raycast.hip -- the resident TSDF volume of path A (er_tsdf.hip) seen from a pose: per pixel the first front face along the ray, as
// er_odom's record map ({vertex | normal}, camera frame) and as a uint16 depth image.  DESIGN.md 7.13 states the rule, er_raycast_math.h IS
// the rule (the kernel below only supplies the volume to it), tests/raycast_restatement.py restates it in numpy and the device is held to
// that restatement bit for bit.
//
// k_raycast: one thread per pixel, a wave = an 8 x 8 pixel tile, a workgroup = 2 x 2 tiles.  The march is a chain of dependent gathers of
// one float2 {sdf, weight}: the vector L1 pays per distinct address (profiles/r06y_gather_rates.txt), and the rays of neighbouring pixels
// visit neighbouring voxels, so a square tile shares more lines than a row of 64 pixels would.  Each lane remembers the key and pool slot
// of the unit it sampled last: the hash map is probed once per unit entered, not once per sample.  Where that unit does not exist the loop
// index advances by the number of steps that provably stay inside the unit's box (er_rc::skip_steps): the trip count is an integer that
// only grows, and the samples that are left out are unobserved whichever way they are counted, so the output is the plain march's.
// The kernel only reads the volume: no atomics, no LDS.  Nobody has measured it yet (scripts/raycast_probe.py is there for that).
//
// k_raycast_batch: the same body for a LIST of jobs (er_tsdf_raycast_batch) -- job = (volume, image, pose, outputs), one per
// blockIdx.z, read once from a table in device memory (the index is the workgroup's, so the reads are scalar).  x and y of the grid are
// sized for the largest image of the list; the workgroups that lie outside a smaller image leave at once.
#include "er_tsdf_dev.h"
#include "er_raycast_math.h"
#include "er_cloud.h"

#include <mutex>

namespace {

using namespace er_tsdf_k;

constexpr int kTilePx = 8;                    // a wave's tile is kTilePx x kTilePx pixels
constexpr int kGroupPx = 2 * kTilePx;         // a workgroup's is 2 x 2 of them

static_assert(er_rc::kLattice == kLatticeVox, "one lattice");

struct DeviceVol {
  VolumeView vol;
  int max_units;
  int ckey, cslot;                            // the unit sampled last (ckey = kEmptyKey: none yet) and its slot, < 0 = it does not exist
  int ux, uy, uz;                             // its lattice position

  __device__ __forceinline__ bool fetch(int gx, int gy, int gz, float& F) {
    if (!on_lattice(gx, gy, gz)) return false;
    const int key = unit_key_of(gx, gy, gz);
    if (key != ckey) {
      const int s = vol.map.slot(key);
      ckey = key;
      cslot = s < max_units ? s : -1;
      ux = gx >> 6, uy = gy >> 6, uz = gz >> 6;
    }
    if (cslot < 0) return false;
    const float2 v = vol.unit(cslot)[unit_offset_of(gx, gy, gz)];
    F = v.x;
    return v.y != 0.0f;
  }

  // (called right after an unobserved nearest-voxel sample at p: if that sample reached a unit at all, it is the cached one)
  __device__ __forceinline__ int advance(float px, float py, float pz, float step) {
    int gx, gy, gz;
    if (!(er_rc::nearest_index(px, gx) & er_rc::nearest_index(py, gy) & er_rc::nearest_index(pz, gz))) return 1;
    if (cslot >= 0 || ckey != unit_key_of(gx, gy, gz)) return 1;
    return er_rc::skip_steps(px, py, pz, ux, uy, uz, step);
  }
};

__global__ __launch_bounds__(kGroupPx * kGroupPx) void k_raycast(VolumeView volume, int max_units, er_rc::Image I, int cols, int rows,
                                                                 float4* __restrict__ rec, uint16_t* __restrict__ depth) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = blockIdx.x * kGroupPx + (wave & 1) * kTilePx + (lane & 7);
  const int v = blockIdx.y * kGroupPx + (wave >> 1) * kTilePx + (lane >> 3);
  if (u >= cols || v >= rows) return;
  DeviceVol vol{volume, max_units, kEmptyKey, -1, 0, 0, 0};
  er_rc::Pixel px;
  er_rc::cast_pixel(vol, I, u, v, px);
  const size_t i = (size_t)v * cols + u;
  if (rec) {
    rec[2 * i] = make_float4(px.v[0], px.v[1], px.v[2], 0.0f);
    rec[2 * i + 1] = make_float4(px.n[0], px.n[1], px.n[2], 0.0f);
  }
  if (depth) depth[i] = px.depth;
}

// One job of k_raycast_batch: what k_raycast takes as arguments.
struct RayJob {
  VolumeView vol;
  float4* rec;
  uint16_t* depth;
  int max_units, cols, rows;
  er_rc::Image I;
};
static_assert(sizeof(RayJob) == 136, "five pointers, five ints and the image: the job table is read with scalar loads, keep it small");

__global__ __launch_bounds__(kGroupPx * kGroupPx) void k_raycast_batch(const RayJob* __restrict__ jobs) {
  const RayJob& J = jobs[blockIdx.z];
  const int cols = J.cols, rows = J.rows;
  if ((int)blockIdx.x * kGroupPx >= cols || (int)blockIdx.y * kGroupPx >= rows) return;     // (workgroup-uniform) a smaller image than the list's largest
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = blockIdx.x * kGroupPx + (wave & 1) * kTilePx + (lane & 7);
  const int v = blockIdx.y * kGroupPx + (wave >> 1) * kTilePx + (lane >> 3);
  if (u >= cols || v >= rows) return;
  DeviceVol vol{J.vol, J.max_units, kEmptyKey, -1, 0, 0, 0};
  const er_rc::Image I = J.I;
  float4* __restrict__ rec = J.rec;
  uint16_t* __restrict__ depth = J.depth;
  er_rc::Pixel px;
  er_rc::cast_pixel(vol, I, u, v, px);
  const size_t i = (size_t)v * cols + u;
  if (rec) {
    rec[2 * i] = make_float4(px.v[0], px.v[1], px.v[2], 0.0f);
    rec[2 * i + 1] = make_float4(px.n[0], px.n[1], px.n[2], 0.0f);
  }
  if (depth) depth[i] = px.depth;
}

constexpr int kMaxJobs = 65535;               // jobs sit on blockIdx.z

// The job table of er_tsdf_raycast_batch: a page-locked block and its device twin, grow-only, one pair per process; a call holds the lock
// from the first entry it writes until its stream is drained.
struct JobTable {
  std::mutex lock;
  int device = -1;
  er::PinnedBuffer<RayJob> host;
  er::Buffer<RayJob> dev;
};
JobTable& job_table() {
  static JobTable* t = new JobTable();     // intentionally leaked: its memory is never freed behind the HIP runtime's back at exit
  return *t;
}

int job_table_reserve(JobTable& t, int device, size_t n) {
  if (t.device == device && n <= t.dev.capacity()) return 0;
  t.host.reset();                                        // (another device's table goes whatever its size)
  t.dev.reset();
  t.device = -1;
  const size_t cap = std::max<size_t>(n, 256);
  if (t.host.reserve(cap, "er_tsdf_raycast_batch") || t.dev.reserve(cap, "er_tsdf_raycast_batch")) {
    t.dev.reset();
    return 1;
  }
  t.device = device;
  return 0;
}

}  // namespace

extern "C" {

int er_raycast_params_default(er_raycast_params* p) {
  if (!p) return er::fail("er_raycast_params_default: NULL argument");
  p->t_min = 0.0f;
  p->t_max = 4.0f;
  p->step = 0.8f * 0.03f;
  return 0;
}

int er_tsdf_raycast(er_tsdf_t h, int cols, int rows, const float cam4[4], const double T[16], const er_raycast_params* params, void* rec_out,
                    uint16_t* depth_out, int out_on_device) {
  const char* who = "er_tsdf_raycast";
  if (!cam4 || !T) return er::fail("%s: NULL argument", who);
  if (cols <= 0 || rows <= 0 || cols > 16384 || rows > 16384) return er::fail("%s: an image of %d x %d (1 .. 16384 each way)", who, cols, rows);
  er_raycast_params P;
  er_raycast_params_default(&P);
  if (params) P = *params;
  int n_steps = 0;
  const int bad = er_rc::count_steps(P.t_min, P.t_max, P.step, &n_steps);
  if (bad == 1) return er::fail("%s: t_min, t_max and step must be finite and step positive", who);
  if (bad == 2) return er::fail("%s: more than %d steps between t_min and t_max", who, er_rc::kMaxSteps);
  for (int i = 0; i < 4; i++)
    if (!std::isfinite(cam4[i])) return er::fail("%s: cam4 is not finite", who);
  if (cam4[0] == 0.0f || cam4[1] == 0.0f) return er::fail("%s: a focal length of 0", who);
  if (!rec_out && !depth_out) return er::fail("%s: both outputs are NULL", who);
  if (!h) return er::fail("%s: NULL handle", who);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (check_flags(h)) return 1;                          // behind every queued batch, like the extraction calls (joins the voxel stream)
  er_rc::Image I;
  er_rc::make_image(cam4, T, P.t_min, P.step, n_steps, I);
  const size_t npix = (size_t)cols * rows;
  float4* d_rec = out_on_device ? (float4*)rec_out : nullptr;
  uint16_t* d_depth = out_on_device ? depth_out : nullptr;
  er::DevScope own;
  char* tmp = nullptr;                                   // host outputs: one device temporary, records then depth
  if (!out_on_device) {
    if (own.alloc(&tmp, npix * (2 * sizeof(float4) + sizeof(uint16_t)), who)) return 1;
    if (rec_out) d_rec = (float4*)tmp;
    if (depth_out) d_depth = (uint16_t*)(tmp + npix * 2 * sizeof(float4));
  }
  hipLaunchKernelGGL(k_raycast, dim3((cols + kGroupPx - 1) / kGroupPx, (rows + kGroupPx - 1) / kGroupPx), dim3(kGroupPx * kGroupPx), 0, h->stream,
                     h->view(), h->max_units, I, cols, rows, d_rec, d_depth);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !out_on_device && rec_out) e = hipMemcpyAsync(rec_out, d_rec, npix * 2 * sizeof(float4), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && !out_on_device && depth_out) e = hipMemcpyAsync(depth_out, d_depth, npix * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return er::fail("%s: %s", who, hipGetErrorString(e));
  return 0;
}

int er_tsdf_raycast_batch(int n_jobs, const er_tsdf_t* vol, const int* cols, const int* rows, const float* cam4, const double* T,
                          const er_raycast_params* params, void* const* rec_out_dev, uint16_t* const* depth_out_dev) {
  const char* who = "er_tsdf_raycast_batch";
  if (n_jobs < 0) return er::fail("%s: n_jobs = %d is negative", who, n_jobs);
  if (n_jobs == 0) return 0;
  if (n_jobs > kMaxJobs) return er::fail("%s: %d jobs, at most %d in one call", who, n_jobs, kMaxJobs);
  if (!vol || !cols || !rows || !cam4 || !T) return er::fail("%s: NULL argument", who);
  // every refusal of er_tsdf_raycast, per job, before anything is launched
  std::vector<int> n_steps((size_t)n_jobs);
  int max_cols = 0, max_rows = 0;
  for (int j = 0; j < n_jobs; j++) {
    if (!vol[j]) return er::fail("%s: job %d: NULL handle", who, j);
    if (vol[j]->device != vol[0]->device)
      return er::fail("%s: job %d: its volume is on device %d, job 0's on device %d (one device per call)", who, j, vol[j]->device, vol[0]->device);
    if (cols[j] <= 0 || rows[j] <= 0 || cols[j] > 16384 || rows[j] > 16384)
      return er::fail("%s: job %d: an image of %d x %d (1 .. 16384 each way)", who, j, cols[j], rows[j]);
    er_raycast_params P;
    er_raycast_params_default(&P);
    if (params) P = params[j];
    const int bad = er_rc::count_steps(P.t_min, P.t_max, P.step, &n_steps[(size_t)j]);
    if (bad == 1) return er::fail("%s: job %d: t_min, t_max and step must be finite and step positive", who, j);
    if (bad == 2) return er::fail("%s: job %d: more than %d steps between t_min and t_max", who, j, er_rc::kMaxSteps);
    for (int i = 0; i < 4; i++)
      if (!std::isfinite(cam4[4 * (size_t)j + i])) return er::fail("%s: job %d: cam4 is not finite", who, j);
    if (cam4[4 * (size_t)j] == 0.0f || cam4[4 * (size_t)j + 1] == 0.0f) return er::fail("%s: job %d: a focal length of 0", who, j);
    if (!(rec_out_dev && rec_out_dev[j]) && !(depth_out_dev && depth_out_dev[j])) return er::fail("%s: job %d: both outputs are NULL", who, j);
    max_cols = std::max(max_cols, cols[j]);
    max_rows = std::max(max_rows, rows[j]);
  }
  const int device = vol[0]->device;
  ER_HIP_TRY(hipSetDevice(device));
  // Behind every queued batch of every volume named: check_flags joins the volume's voxel stream and waits for it, so whatever this call
  // launches afterwards, on any stream, stands behind the volume's last integration.
  for (int j = 0; j < n_jobs; j++) {
    bool seen = false;
    for (int q = 0; q < j && !seen; q++) seen = vol[q] == vol[j];
    if (!seen && check_flags(vol[j])) return 1;
  }
  std::lock_guard<std::mutex> guard(job_table().lock);
  JobTable& jobs = job_table();
  if (job_table_reserve(jobs, device, (size_t)n_jobs)) return 1;
  for (int j = 0; j < n_jobs; j++) {
    er_raycast_params P;
    er_raycast_params_default(&P);
    if (params) P = params[j];
    er_tsdf_t h = vol[j];
    RayJob& J = jobs.host[j];
    J.vol = h->view();
    J.rec = rec_out_dev ? (float4*)rec_out_dev[j] : nullptr;
    J.depth = depth_out_dev ? depth_out_dev[j] : nullptr;
    J.max_units = h->max_units;
    J.cols = cols[j];
    J.rows = rows[j];
    er_rc::make_image(cam4 + 4 * (size_t)j, T + 16 * (size_t)j, P.t_min, P.step, n_steps[(size_t)j], J.I);
  }
  er::StreamLease lease;                                   // a stream of the call's own; its destructor drains it
  if (lease.acquire(device)) return 1;
  hipStream_t st = lease.stream;
  ER_HIP_TRY(hipMemcpyAsync(jobs.dev, jobs.host, sizeof(RayJob) * (size_t)n_jobs, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_raycast_batch, dim3((max_cols + kGroupPx - 1) / kGroupPx, (max_rows + kGroupPx - 1) / kGroupPx, n_jobs), dim3(kGroupPx * kGroupPx),
                     0, st, jobs.dev);
  ER_HIP_TRY(hipGetLastError());
  ER_HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"

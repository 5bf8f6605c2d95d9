// er_tsdf_int.hip -- path A's voxel pass, k_integrate: a file of its own so that it can have compiler flags of its own (Makefile:
// FLAGS_er_tsdf_int.hip; er_tsdf.h says why).  er_tsdf.hip launches it (run_batch).
#include "er_tsdf.h"

namespace er_tsdf_k {

// ------------------------------------------------------------------------------------------------
// IntegrateVolumeUnit (TSDFVolume.cpp:69-102) for every touched unit of the batch.
// Work item = 1024 voxels of a unit for one 256-thread workgroup (256 items per unit); each wave owns 256 of them in kRows = 4 register rows of 64 -- a
// 8 x 4 x 8 box (mapping below).  The voxels stay in registers while the wave walks the unit's frame mask in ASCENDING frame order (wave-uniform loop:
// the frame constants arrive by scalar loads) -- per voxel exactly the reference's frame-by-frame sequence.
// Items come from ONE global work queue in cost order (k_plan), claimed when the workgroup is free.  (Static deals, per-XCD queues and look-ahead
// claims were all measured slower: profiles/HISTORY.md "Path A: the schedule of k_integrate".)
// kSure: the square-root-free "sure" path of the frame loop (voxel_classify needs dp < 64 m; the host picks the instantiation
// from integration_trunc, which bounds every scaled depth).
template <bool kSure>
__global__ __launch_bounds__(kBlock, kIntMinBlocks) void k_integrate(
    float2* __restrict__ pool, const PlanRec* __restrict__ plan_rec, Plan* __restrict__ plan,
    const FrameXform* __restrict__ frames, const float* __restrict__ scaled, const float* __restrict__ tile_max,
    const float* __restrict__ tile_lo, const float* __restrict__ tile_lo_fine, int tiles_x, int tiles_y, Camera cam, int cols, int rows) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int pixels = cols * rows;
  const int lo_tiles_x = (cols + (1 << kLoShift) - 1) >> kLoShift;
  const int n_items = plan->n_units * kItemsPerUnit;
  // Work queue: the items are sorted by descending cost (k_plan) and every workgroup claims the next one when it is done with its own (one atomic per
  // item and workgroup; 3 persistent workgroups per CU): longest-processing-time-first.  The culling and the full / sure shortcuts make the real cost of
  // an item unpredictable; with a static deal the kernel lasted as long as its unluckiest workgroup.  Two barriers per item on purpose: they keep the
  // four boxes of an item -- neighbours in the volume, hence in every depth image -- in step on one CU (barrier-free hand-outs measured 1.7 x the time
  // per frame visit, profiles/r05m_*).
  __shared__ int s_item;
  for (;;) {
    __syncthreads();                                                     // everybody is done with the previous s_item
    if (threadIdx.x == 0) s_item = atomicAdd(&plan->next, 1);
    __syncthreads();
    const int item = s_item;
    if (item >= n_items) break;
    const PlanRec rec = plan_rec[item >> 8];                              // (wave-uniform: one 16-byte scalar load)
    // The wave owns a COMPACT 8 x 4 x 8 BOX of the unit.  Lanes = 2 slabs x 4 x 8 voxels (il, jl, kl), register row r = the next pair of slabs
    // (i = i0 + il + 2 r); the workgroup's item = 8 x 8 x 16 voxels (waves: 2 along j, 2 along k).  Why this shape: a depth gather costs the vector L1
    // ~0.6 clocks per DISTINCT address (profiles/r06y_gather_rates.txt) and k_integrate lives on its gathers (every gather issued twice: -19 % frames/s,
    // profiles/r06z_ab_lane_shape.txt); the 64 voxels of an 8 x 8 plane -- rounds 2-5: lanes = one slab, rows = 4 slabs -- project onto 64 distinct pixels
    // seen face-on, a 2 x 4 x 8 block onto fewer from every direction.  +4 % on the job against the 1 x 8 x 8 lanes; 4 x 4 x 4, 2 x 8 x 4, 2 x 2 x 16, 4 x 2 x 8, 1 x 4 x 16 lanes and two other item shapes measured behind it.  A compact box keeps a tight
    // pixel hull (culling, the "inside" verdict), few idle lanes at surfaces and frustum borders and few patches that cross a surface; four rows per lane
    // keep the longest items short and the kernel at 93 VGPRs.  Voxel accesses: eight 8-byte voxels = one 64-byte segment per (il, jl).
    const int ilane = lane >> 5;
    const int i = ((item >> 5) & 7) * 8 + ilane;
    const int j0 = ((item >> 2) & 7) * 8 + (wave >> 1) * 4;
    const int jlane = (lane >> 3) & 3, k0 = (item & 3) * 16 + (wave & 1) * 8, klane = lane & 7;
    constexpr int jspan = 4, kspan = 8, ispan = 2 * kRows, istep = 2;
    const int ibox = i - ilane;                                          // (wave-uniform: the box's first slab)
    const int key = rec.key, slot = rec.slot;
    if (slot < 0) continue;                                             // pool overflow: reported by the host
    unsigned long long m = rec.mask;
    const int xi = key >> 18, yi = (key >> 9) & 511, zi = key & 511;
    const float xs = unit_shift(xi), ys = unit_shift(yi), zs = unit_shift(zi);
    const float g2 = grid_coord(k0 + klane, zs);
    float2* __restrict__ slab = pool + (size_t)slot * kUnitVox + (size_t)i * (kUnitRes * kUnitRes) + (j0 + jlane) * kUnitRes + k0 + klane;
    float S[kRows], W[kRows], W0[kRows], g0[kRows];                      // g0 per register row and slab of the lane, g1 / g2 per lane
    const float g1 = grid_coord(j0 + jlane, ys);
#pragma unroll
    for (int r = 0; r < kRows; r++) g0[r] = grid_coord(i + r * istep, xs);
    constexpr int row_stride = istep * kUnitRes * kUnitRes;
#pragma unroll
    for (int r = 0; r < kRows; r++) {                                   // loads in flight while the culling preamble computes
      const float2 v = slab[r * row_stride];                      // (loading only the surviving patches, after the culling,
      S[r] = v.x;                                                       //  was measured: no change, the kernel is VALU-bound --
      W[r] = v.y;                                                       //  profiles/r02f_ab_k_integrate_variants.txt)
      W0[r] = v.y;
    }
    // Exact culling: lane f tests frame f of the batch against this wave's patch of 256 voxels; frames that
    // provably cannot update any voxel of the patch leave the mask (er_tsdf_math.h: patch_may_update).
    // The same test also tells which of the remaining frames see the WHOLE patch inside the image and clear of the camera
    // plane (m_in): for those the per-voxel range tests are proven true and the loop below skips them.
    // Third verdict (m_full): the frame updates EVERY voxel of the patch with tsdf = 1 -- proven from the tile minima of the depth
    // under the patch's pixel hull -- so the frame needs no projection, no depth sample and no arithmetic at all: W += 1, and S
    // stays / becomes exactly 1 wherever S == 1 or W == 0 (most of the frustum is such free space).
    unsigned long long m_in, m_full;
    {
      bool keep = ((m >> lane) & 1ull) != 0ull, inside = false, full = false;
      // lane f tests frame f: its 16 constants come from the component-major copy behind frames[] (Staging::fxT) -- 64 lanes x 4 consecutive bytes per
      // load where frames[lane] is one 64-byte line per lane
      FrameXform fl;
      if (keep) {
        const float* __restrict__ fT = reinterpret_cast<const float*>(frames + ER_MAX_BATCH) + lane;
#pragma unroll
        for (int q = 0; q < 12; q++) fl.mi[q] = fT[q * ER_MAX_BATCH];
        fl.tx = fT[12 * ER_MAX_BATCH];
        fl.ty = fT[13 * ER_MAX_BATCH];
        fl.tz = fT[14 * ER_MAX_BATCH];
        fl.pad = 0.f;
      }
      if (keep)
        keep = patch_may_update_box(grid_coord(ibox, xs), grid_coord(ibox + ispan - 1, xs), grid_coord(j0, ys), grid_coord(j0 + jspan - 1, ys),
                                    grid_coord(k0, zs), grid_coord(k0 + kspan - 1, zs), fl, cam, cols, rows,
                                    // tiles FRAME-fastest: lane f of this test is frame f, and consecutive frames of a sweep see the box under the
                                    // same tiles -- 64 lanes x 4 consecutive bytes per load instead of 64 lines 1.2 KB apart
                                    tile_max + lane, tiles_x, tiles_y, &inside, tile_lo + lane, &full, kLoShift, lo_tiles_x, tile_lo_fine + lane,
                                    ER_MAX_BATCH);
      m = __ballot(keep);
      m_in = __ballot(keep && inside);
      m_full = __ballot(keep && full);
    }
    // Frame loop in two halves: project() computes the pixel under every voxel of the four register rows and issues the depth
    // gathers, finish() does the arithmetic that needs the samples; the loop below overlaps the two halves of consecutive frames.
    auto project = [&](int f, float (&dp)[kRows]) {
      const FrameXform fx = frames[f];
      const float* __restrict__ sc = scaled + (size_t)f * (pixels + kScaledPad);
      unsigned pix[kRows];
      if ((m_in >> f) & 1ull) {                                          // wave-uniform
#pragma unroll
        for (int r = 0; r < kRows; r++) pix[r] = voxel_project_inside(g0[r], g1, g2, fx, cam, cols, rows);
      } else
      {
#pragma unroll
        for (int r = 0; r < kRows; r++) {
          unsigned pixel;
          const bool ok = voxel_project(g0[r], g1, g2, fx, cam, cols, rows, pixel);
          pix[r] = ok ? pixel : (unsigned)pixels;                        // the frame's zero pad: dp = 0 fails ":82 dp > 0.001" like the reference's early out
        }
      }
      // kRows UNCONDITIONAL gathers in straight-line code after the branches, nothing that depends on them here: the wait in
      // finish() is then "all but the newest kRows loads" on every path (predicated loads or loads inside the branches make the
      // count path-dependent and the compiler falls back to waiting for everything)
#pragma unroll
      for (int r = 0; r < kRows; r++) dp[r] = sc[pix[r]];
    };
    auto finish = [&](int f, const float (&dp)[kRows]) {
      const FrameXform& fx = frames[f];                                  // (only the camera centre: three scalar loads)
      float d2[kRows];
#pragma unroll
      for (int r = 0; r < kRows; r++) d2[r] = voxel_dist2(g0[r], g1, g2, fx);
      if (kSure) {
        // Sure path (er_tsdf_math.h: voxel_classify): if every lane of the four rows is provably in free space (tsdf = 1) or
        // provably behind the surface (no update) and every free lane holds S == 1 or W == 0, the whole update of this frame is
        // "W += 1, S = 1" on the free lanes -- no square root, no band quotient, no division.  78 % of the (patch, frame)
        // visits of the golden scene; one wave-uniform branch per frame.
        bool fre[kRows], need = false;
#pragma unroll
        for (int r = 0; r < kRows; r++) {
          bool behind;
          voxel_classify(dp[r], d2[r], fre[r], behind);
          need = need | !(fre[r] | behind) | (fre[r] & !voxel_free_trivial(S[r], W[r]));
        }
        if (__ballot(need) == 0ull) {
#pragma unroll
          for (int r = 0; r < kRows; r++) {
            S[r] = fre[r] ? 1.0f : S[r];
            W[r] = fre[r] ? W[r] + 1.0f : W[r];
          }
          return;
        }
      }
#pragma unroll
      for (int r = 0; r < kRows; r++) {
        const bool upd = voxel_finish_d2(S[r], W[r], dp[r], d2[r]);
        (void)upd;
      }
    };
    // Software pipeline over the frames that need a projection: the projection and the four depth gathers of the NEXT such frame are issued before the
    // current frame's samples are used (a wave used to sit on its gathers once per frame: 3100 ticks per visit for ~730 issue cycles).  Runs of full
    // frames need no samples and are applied where they fall in the ascending order, so every voxel still sees its frames one by one in frame order.
    // Two stages per trip with alternating sample registers (a rotating copy would have to wait for the data it copies); the last frame is finished
    // after the loop.  +4 % for the job together with three instead of four persistent workgroups per CU (profiles/r05n_ab_frame_pipeline.txt).
    {
      unsigned long long mn = m & ~m_full, mf = m & m_full;
      auto apply_full = [&](unsigned long long run) {
        const int n = __popcll(run);
        bool nontrivial = false;
#pragma unroll
        for (int r = 0; r < kRows; r++) nontrivial = nontrivial | !(voxel_free_trivial(S[r], W[r]) & (W[r] < 8388608.0f));
        if (__ballot(nontrivial) == 0ull) {                              // (S W + 1) / (W + 1) == 1 exactly, W + n exact below 2^24
#pragma unroll
          for (int r = 0; r < kRows; r++) {
            S[r] = 1.0f;
            W[r] = W[r] + (float)n;
          }
        } else {                                                         // a voxel that was inside the truncation band before: the n divisions, in order
          for (int q = 0; q < n; q++) {
#pragma unroll
            for (int r = 0; r < kRows; r++) {
              S[r] = div_inrange(S[r] * W[r] + 1.0f, W[r] + 1.0f);
              W[r] = W[r] + 1.0f;
            }
          }
        }
      };
      auto runs_before = [&](int f) {
        const unsigned long long run = f < 64 ? (mf & ((1ull << f) - 1ull)) : mf;   // the full frames before the next projected one
        if (run) {                                                       // wave-uniform
          mf &= ~run;
          apply_full(run);
        }
      };
      if (mn) {
        float dpa[kRows], dpb[kRows];
        int pf = __builtin_ctzll(mn);
        mn &= mn - 1;
        project(pf, dpa);
        bool last_in_b = false;
        for (;;) {                                                       // two stages per trip: the sample registers alternate; the last frame is finished after the loop
          runs_before(pf);
          if (mn == 0ull) break;                                         // (pf's samples are in dpa)
          int nf = __builtin_ctzll(mn);
          mn &= mn - 1;
          project(nf, dpb);
          finish(pf, dpa);
          pf = nf;
          runs_before(pf);
          if (mn == 0ull) {                                              // (pf's samples are in dpb)
            last_in_b = true;
            break;
          }
          nf = __builtin_ctzll(mn);
          mn &= mn - 1;
          project(nf, dpa);
          finish(pf, dpb);
          pf = nf;
        }
        float dpl[kRows];
#pragma unroll
        for (int r = 0; r < kRows; r++) dpl[r] = last_in_b ? dpb[r] : dpa[r];
        finish(pf, dpl);                                                 // the last projected frame: nothing left to prefetch
      }
      runs_before(64);                                                   // the full frames after the last projected one
    }
#pragma unroll
    for (int r = 0; r < kRows; r++)
      if (W[r] != W0[r]) slab[r * row_stride] = make_float2(S[r], W[r]);
  }
}
template __global__ void k_integrate<true>(float2* __restrict__, const PlanRec* __restrict__, Plan* __restrict__, const FrameXform* __restrict__, const float* __restrict__, const float* __restrict__, const float* __restrict__, const float* __restrict__, int, int, Camera, int, int);
template __global__ void k_integrate<false>(float2* __restrict__, const PlanRec* __restrict__, Plan* __restrict__, const FrameXform* __restrict__, const float* __restrict__, const float* __restrict__, const float* __restrict__, const float* __restrict__, int, int, Camera, int, int);

}  // namespace er_tsdf_k

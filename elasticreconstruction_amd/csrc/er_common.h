// er_common.h -- shared host-side helpers of liber_hip.so (error reporting, HIP call checking,
// small row-major 4x4 double algebra).  No torch, no Eigen: the system has no linear-algebra
// library outside /root/reference, and the C ABI must stay plain C.
#pragma once

#include <hip/hip_runtime.h>

#include "er_mat4.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace er {

// Thread-local error text behind er_last_error().
char* error_buffer();
int fail(const char* fmt, ...);

#define ER_HIP_TRY(expr)                                                                          \
  do {                                                                                            \
    hipError_t er_e_ = (expr);                                                                    \
    if (er_e_ != hipSuccess)                                                                      \
      return ::er::fail("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr, hipGetErrorString(er_e_)); \
  } while (0)

// The same for code shared by several entry points: the text names the entry point `who` instead of the file and line.
#define ER_W(who, expr)                                                                         \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return ::er::fail("%s: %s failed: %s", who, #expr, hipGetErrorString(e_)); \
  } while (0)

}  // namespace er

// internal accessors of a TSDF handle for the other translation units of the library (not part of the C ABI)
struct er_tsdf_s;
namespace er {
hipStream_t tsdf_stream(er_tsdf_s* h);
int tsdf_device(er_tsdf_s* h);
}  // namespace er

// er_odom.hip for the fragment builder (er_fragments.hip): er_odom_align_pairs' loop over ANY pair list whose model side may name one of n_models
// models (model k = "frame" n_frames + k; model_rec_dev[k * levels + l] in device memory), and the handle's level count.
struct er_odom_s;
namespace er {
__attribute__((visibility("hidden"))) int odom_align_models(er_odom_s* h, const char* who, int n_models, const void* const* model_rec_dev, int n_frames,
                                                            const uint16_t* depth, int on_device, int n_pairs, const int* model_idx, const int* frame_idx,
                                                            const double* guess, double* T_out, int* status, double* trace, double* sums, int window);
__attribute__((visibility("hidden"))) int odom_levels(er_odom_s* h);
}  // namespace er

// er_cloud_create for rows that already live on `device` (er_cloud_create_from_tsdf): xyz_dev / normal_dev are packed [n][3] float arrays in
// device memory whose contents are complete (their producer's stream has been synchronised); they are free again when the call returns.
// (Declared here for er_tsdf_extract.hip; the rest of what path B's translation units share is er_cloud.h.)
struct er_cloud_s;
namespace er {
int cloud_create_device(const float* xyz_dev, const float* normal_dev, int n, float grid_cell, int device, er_cloud_s** out);
}  // namespace er

// launch.h -- the launch entry points of the .hip files, declared once for capi.cpp and for the files
// that define them: with C linkage only the compiler can hold a definition to its declaration.
#pragma once
#include <hip/hip_runtime.h>

#include "accumulate.h"
#include "denoise.h"
#include "denoise_variance.h"
#include "engine.h"
#include "guides.h"
#include "texels.h"

extern "C" {
// render.hip
hipError_t atr_launch_render(const atr::RenderParams& P, int sched, int primary_occ, hipStream_t s);
int atr_render_reads_pads(const atr::RenderParams& P, int sched);
hipError_t atr_launch_camera_pads(const atr::DScene* scene, const atr::PadEyes& eyes, int32_t nrows, int32_t stride,
                                  int fold, int wide, atr::float2_t* table, atr::float2_t* info, atr::float4_t* boxes,
                                  float* edges, hipStream_t s);
hipError_t atr_launch_camera_leaf_boxes(const atr::DScene* scene, const atr::PadEyes& eyes, int32_t nrows, int32_t stride,
                                        int wide, const atr::float2_t* pads, int32_t lstride, atr::float4_t* lbox,
                                        hipStream_t s);
hipError_t atr_launch_traced_finish(unsigned long long* slots, unsigned long long* out, hipStream_t s);
hipError_t atr_launch_unpack(const atr::DBlock* blocks, int32_t nblocks, int32_t width, const uint32_t* packed,
                             uint32_t* image, hipStream_t s);
hipError_t atr_launch_tile_casts(const atr_tile* tiles, int32_t ntiles, int32_t width, const uint32_t* casts,
                                 int64_t* out, hipStream_t s);
hipError_t atr_launch_packed_tile_casts(const int32_t* slot_tile, int64_t nslots, const uint32_t* casts,
                                        int64_t frame_stride, int32_t nframes, int32_t ntiles,
                                        unsigned long long* out, hipStream_t s);
// paths.hip
hipError_t atr_launch_path_camera(const atr::PathParams& P, int occ, hipStream_t s);
hipError_t atr_launch_path_bounce(const atr::PathParams& P, int ncu, int occ, hipStream_t s);
hipError_t atr_launch_path_resolve(const atr::PathParams& P, hipStream_t s);
hipError_t atr_launch_path_sort(const atr::PathParams& P, int ncu, hipStream_t s);
hipError_t atr_launch_path_live(const atr::PathParams& P, hipStream_t s);
hipError_t atr_launch_path_camera_adaptive(const atr::PathParams& P, int ncu, hipStream_t s);
hipError_t atr_launch_path_resolve_adaptive(const atr::PathParams& P, hipStream_t s);
hipError_t atr_launch_sort_bins(const atr::PathSort& so, hipStream_t s);  // also the ray queries' (query.hip)
// query.hip, occlusion.hip
hipError_t atr_launch_query_sort(const atr::QueryParams& P, int ncu, hipStream_t s);
hipError_t atr_launch_query(const atr::QueryParams& P, int lane, int ncu, hipStream_t s);
hipError_t atr_launch_occlusion(const atr::OcclParams& P, int lane, int ncu, hipStream_t s);
// gather.hip
hipError_t atr_launch_gather(const atr::GatherParams& P, int lane, int ncu, hipStream_t s);
// radiance.hip
hipError_t atr_launch_radiance_entry(const atr::RadianceParams& P, int ncu, hipStream_t s);
hipError_t atr_launch_radiance_resolve(const atr::RadianceParams& P, hipStream_t s);
// gather_radiance.hip
hipError_t atr_launch_gather_radiance_entry(const atr::GatherRadianceParams& P, int ncu, hipStream_t s);
hipError_t atr_launch_gather_radiance_resolve(const atr::GatherRadianceParams& P, hipStream_t s);
// probe_sh.hip
hipError_t atr_launch_probe_sh_entry(const atr::ProbeShParams& P, int ncu, hipStream_t s);
hipError_t atr_launch_probe_sh_resolve(const atr::ProbeShParams& P, hipStream_t s);
// texels.hip
hipError_t atr_launch_texel_classify(const atr::TexelParams& P, hipStream_t s);
hipError_t atr_launch_texel_big(const atr::TexelParams& P, uint32_t nbig, hipStream_t s);
hipError_t atr_launch_texel_scan(const atr::TexelParams& P, hipStream_t s);
hipError_t atr_launch_texel_write(const atr::TexelParams& P, hipStream_t s);
hipError_t atr_launch_texel_scatter(const float* values, const int32_t* texel, int64_t n, int64_t ntexels, float* image,
                                    uint8_t* flag, hipStream_t s);
hipError_t atr_launch_texel_dilate(const atr::TexelImageParams& P, hipStream_t s);
hipError_t atr_launch_texel_fill(const atr::TexelImageParams& P, hipStream_t s);
// denoise.hip
hipError_t atr_launch_denoise_pack(const atr::DenoisePack& P, hipStream_t s);
hipError_t atr_launch_denoise_pass(const atr::DenoisePass& P, int normal, int position, int colour, hipStream_t s);
// denoise_variance.hip
hipError_t atr_launch_denoise_variance_pack(const atr::DenoiseVarPack& P, hipStream_t s);
hipError_t atr_launch_denoise_variance_estimate(const atr::DenoiseVarEstimate& P, int normal, int position, hipStream_t s);
hipError_t atr_launch_denoise_variance_pass(const atr::DenoiseVarPass& P, int normal, int position, int luminance,
                                            hipStream_t s);
// accumulate.hip
hipError_t atr_launch_accumulate(const atr::AccumulateParams& P, hipStream_t s);
// guides.hip
hipError_t atr_launch_camera_guides(const atr::GuidesParams& P, hipStream_t s);
hipError_t atr_launch_camera_rays(const atr::CameraRaysParams& P, hipStream_t s);
// plan.hip
hipError_t atr_launch_plan(const atr::DBlock* base, int32_t nb, unsigned long long* cost,
                           unsigned long long* cost_last, void* work, atr::DBlock* out, int32_t max_split,
                           float split2, float split4, hipStream_t s);
size_t atr_plan_work_bytes(int32_t nb);
// exchange.hip
hipError_t atr_launch_pack_bgr(const uint32_t* src, int64_t n, uint8_t* dst, hipStream_t s);
int64_t atr_masked_chunks(int64_t n);
int atr_unpack_max_sources();
hipError_t atr_launch_unpack_masked_multi(int32_t n, const atr::DBlock* const* blocks, const int32_t* nblocks,
                                          const int64_t* own, const uint8_t* const* in, const int32_t* raw,
                                          int32_t width, int32_t nframes, uint32_t* image, int64_t image_stride,
                                          hipStream_t s);
hipError_t atr_launch_unpack_masked(const atr::DBlock* blocks, int32_t nblocks, int32_t width, const uint8_t* in,
                                    int32_t nframes, int64_t own, uint32_t* image, int64_t image_stride,
                                    hipStream_t s);
hipError_t atr_launch_pack_bgr_masked(const uint32_t* src, int64_t n, uint32_t bg, uint8_t* out, int64_t* nbytes,
                                      hipStream_t s);
hipError_t atr_launch_scatter_bgr_masked(const uint8_t* in, int64_t n, const int64_t* dst_index, uint32_t* image,
                                         hipStream_t s);
hipError_t atr_launch_scatter_bgr(const uint8_t* src, int64_t n, const int64_t* dst_index, uint32_t* image,
                                  hipStream_t s);
}  // extern "C"

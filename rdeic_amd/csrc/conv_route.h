// Host planning of a conv launch (conv_route.cpp): descriptor validation, the route (which kernel family runs)
// and the slicing into image groups / row bands. Host arithmetic only: no device compiler, no HIP runtime, and
// nothing here reads through a descriptor's pointers (their values are used for alignment checks only).
#pragma once
#include <stdint.h>

#include "../../include/rdeic_hip.h"

#ifndef RDEIC_OK
#define RDEIC_OK 0
#define RDEIC_EINVAL (-22)
#endif
#if defined(__HIPCC__)
#define RDEIC_HD __host__ __device__
#else
#define RDEIC_HD
#endif

namespace rdeic_conv {

// process-wide switches (rdeic_set_conv_option / rdeic_set_conv_path)
extern int g_conv_path;     // 0: 128-tiles with the fused GroupNorm prologue only, 2 (default): big-tile auto choice
extern int g_epi_vec;       // LDS-staged vector epilogue (option 0)
extern int g_swz;           // swizzled 128-B LDS rows where they win (1) / padded 144-B rows everywhere (0) (option 3)
extern int g_force_tile;    // >= 0: force launch_plain_auto's candidate (option 4), tuning only
extern int g_dma;           // LDS-DMA path for cin % 64 == 0 (option 5)
extern int g_halo;          // 3x3 halo conv: 0 off, 1 for GroupNorm-input convs (default), 2 for every eligible conv
extern int g_halo8;         // the 8-row halo conv where it applies (option 9)
extern int g_edge;          // the VAE edge kernels where they apply (option 10)
extern int g_up2_phases;    // rdeic_conv2d_up2_phases runs the four folded 2x2 phase convs (option 11)
extern int g_launch_limit;  // largest activation byte span one launch addresses (option 12), <= 2^31 - 1

// Kernel geometry the route depends on (the kernels' own constants are defined from these).
constexpr int HALO_TR = 4, HALO8_TR = 8, HALO_TC = 64;  // output rows / columns per halo tile (4- and 8-row form)
constexpr int HALO_BN = 128;                            // output channels per halo tile
constexpr int HALO_AB_MAX = 512;                        // input channels whose GroupNorm affine fits the LDS table
// Widest GroupNorm-input conv the halo kernel takes over from the materialised path: measured at B=16
// (tools/halo_bench.py, r03) it wins on the 512^2 128-channel layers (2.14 -> 1.53 ms, 3.59 -> 2.62 ms) and the
// 256^2 ones (0.86 -> 0.75, 1.39 -> 1.26 ms) and ties the 256x256 im2col tiles on the 512-channel layers at
// 128^2 / 64^2 (where it still saves the GroupNorm apply launches).
constexpr int HALO_GN_MAX_COUT = 512;
constexpr int NARROW_TR = 8, NARROW_TC = 64;            // the narrow (norm -> SiLU -> conv to <= 16 channels) tile
constexpr int NARROW_LDS = (NARROW_TR + 2) * (NARROW_TC + 2) * 64;  // its halo bytes; table and weights follow
constexpr long MATERIALIZE_SMALLC_PIX = 1l << 20;  // cout <= 4 convs of this many pixels apply their GroupNorm first:
                                                   // the direct kernels redo it for each of the 9 taps

// Whether the LDS-staged vector epilogue can run (A: ConvArgs on the device, rdeic_conv_desc in the planner).
template <class A>
RDEIC_HD inline bool epi_vec_ok(const A& a) {
  if (a.out_mode == 2) return (a.cout % 8) == 0 && (a.out_ld % 4) == 0 && ((uintptr_t)a.out % 8) == 0;
  return a.out_mode == 0 && (a.cout % 8) == 0 && (a.out_ld % 8) == 0 && ((uintptr_t)a.out % 16) == 0 &&
         (!a.res || ((a.res_ld % 8) == 0 && ((uintptr_t)a.res % 16) == 0));
}

// What make_args checks before it fills the kernel arguments: RDEIC_OK or RDEIC_EINVAL.
int validate_desc(const rdeic_conv_desc* d);
// 16-byte gathers: every input segment a multiple of the chunk in channels and pixel stride, 16-byte aligned
bool vec_ok(const rdeic_conv_desc* d);

// ---- image groups and row bands ----
// The fast kernels address activations through 32-bit byte offsets. A launch over several images that exceeds
// g_launch_limit runs as groups of whole images; one image that exceeds it runs as bands of output rows, each band
// a launch of the same kernel over a row window of the input (h, pad_t) and of the output / residual (ho).
long image_span(const rdeic_conv_desc* d);  // the largest of one image's input, output and residual byte spans
// Output rows per band (a multiple of row_tile; with gn_part, of whole 64-row statistic blocks): ho when the image
// fits, 0 when not even one row tile does.
int band_rows(const rdeic_conv_desc* d, int row_tile);
struct Band {
  int r0, rows;   // output rows [r0, r0 + rows)
  int i0, h;      // stored input rows [i0, i0 + h) the band reaches
  int pad_t;      // rows of zero padding above input row i0 (0 for an interior band: it carries its upper rows)
};
Band band_at(const rdeic_conv_desc* d, int r0, int rows);
// Images per launch of the phase path: the largest group whose input span and (4x larger) output span both stay
// inside the launch limit, EVENED OUT over the groups (the other paths take the largest group that fits); 0 when
// one image already exceeds that (it runs as row bands).
int up2_phase_group(const rdeic_conv_desc* d);

// DMA-path eligibility of ONE launch: bf16, 16-byte-aligned 64-channel blocks, every input span inside the launch
// limit. b0 / b1 / bw: the byte extents of the two inputs and the weight (the kernel's buffer descriptors).
bool dma_ok(const rdeic_conv_desc* d, unsigned& b0, unsigned& b1, unsigned& bw);
bool halo_ok(const rdeic_conv_desc* d);
bool halo8_form(const rdeic_conv_desc* d);  // the 8-row halo kernel (else the 4-row one)
bool up2_phases_ok(const rdeic_conv_desc* d, long phase_stride);
// One phase launch's descriptor from a slice s of the upsample conv: the 2x2 conv over the raw input rows of s.
rdeic_conv_desc up2_phase_desc(const rdeic_conv_desc& s);

// A plan: the route and how the conv is cut. Slices are images [i0, i0 + images) x output rows [r0, r0 + rows),
// image groups outermost; every slice of a plan the planner returns is a launch its kernel accepts.
struct Plan {
  int route = RDEIC_ROUTE_DIRECT;
  int images = 0, rows = 0;  // per launch (the last group / band may be shorter)
  int launches = 0;
};
// The route of rdeic_conv2d (tile -2) / rdeic_conv2d_tile (tile >= -1). caller_materializes: answer
// RDEIC_ROUTE_MATERIALIZE where the caller should apply the GroupNorm first (rdeic_conv2d_plan); false: the kernel
// that runs the descriptor as it is (the dispatch). Returns RDEIC_OK or RDEIC_EINVAL.
int plan_conv(const rdeic_conv_desc* d, int tile, bool caller_materializes, Plan& p);
// The phase path's plan (route DMA); false = not eligible.
bool plan_up2_phases(const rdeic_conv_desc* d, long phase_stride, Plan& p);

struct Slice {
  rdeic_conv_desc d;  // the sub-descriptor: n, h, ho, pad_t and every per-pixel / per-image pointer of the slice
  int i0, r0;         // first image, first output row
  long gn_row0;       // absolute output pixel of the slice's first (statistics slot / 64-row block origin)
};
// Slice k of a plan (k < p.launches) over d. The one place a slice's pointers are computed.
Slice slice_at(const rdeic_conv_desc* d, const Plan& p, int k);

}  // namespace rdeic_conv

// Host planning of a conv launch: descriptor validation, the route and the slicing (conv_route.h). Every rule
// that decides which kernel family a descriptor runs on, and how a launch past the launch limit is cut into image
// groups or row bands, lives in this file; the launchers in conv_*.hip only launch what a plan says.
#include "conv_route.h"

namespace rdeic_conv {

int g_conv_path = 2;
int g_epi_vec = 1;
int g_swz = 1;
int g_force_tile = -1;
int g_dma = 1;
int g_halo = 1;
int g_halo8 = 1;
int g_edge = 1;
int g_up2_phases = 1;
int g_launch_limit = 0x7fffffff;

namespace {
long gcd_l(long a, long b) { while (b) { const long t = a % b; a = b; b = t; } return a; }
long lcm_l(long a, long b) { return a / gcd_l(a, b) * b; }
int cdiv_i(long a, long b) { return (int)((a + b - 1) / b); }
bool al16(const void* p) { return ((uintptr_t)p) % 16 == 0; }
int batch_of(const rdeic_conv_desc* d) { return d->batch > 1 ? d->batch : 1; }
int esize(const rdeic_conv_desc* d) { return d->dtype == 0 ? 4 : 2; }
int osize(const rdeic_conv_desc* d) { return (d->out_f32 || d->dtype == 0) ? 4 : 2; }
// bytes of one stored input row / of one output row's pixels (the widest of the tensors addressed with them)
long in_row_bytes(const rdeic_conv_desc* d) {
  const long ld = d->c1 && d->ld1 > d->ld0 ? d->ld1 : d->ld0;
  return (long)d->w * ld * esize(d);
}
long out_row_bytes(const rdeic_conv_desc* d) {
  const long ld = d->res && d->res_ld > d->out_ld ? d->res_ld : d->out_ld;
  return (d->out_mode == 1 ? 4l : 1l) * d->wo * ld * osize(d);
}
bool is_3x3_same(const rdeic_conv_desc* d) {  // 3x3, stride 1, pad 1 over one un-upsampled input
  return d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad_t == 1 && d->pad_l == 1 && !d->up2 && !d->c1 &&
         d->ho == d->h && d->wo == d->w;
}
}  // namespace

int validate_desc(const rdeic_conv_desc* d) {
  if (!d || !d->in0 || !d->weight || !d->out) return RDEIC_EINVAL;
  if (d->c0 <= 0 || d->c1 < 0 || (d->c1 > 0 && !d->in1) || d->cout <= 0 || d->kh <= 0 || d->kw <= 0 ||
      d->stride <= 0 || d->n <= 0 || d->ho <= 0 || d->wo <= 0)
    return RDEIC_EINVAL;
  if (d->dtype != 0 && d->dtype != 1) return RDEIC_EINVAL;
  if ((d->ln_rows != nullptr) != (d->ln_colsum != nullptr)) return RDEIC_EINVAL;
  if (d->ln_rows && (d->dtype != 1 || d->batch > 1 || d->out_mode == 1 || d->gn_ab || !al16(d->ln_colsum)))
    return RDEIC_EINVAL;
  if (d->batch > 1 && (d->res || d->emb || d->out_mode)) return RDEIC_EINVAL;
  if (d->wld < d->kh * d->kw * (d->c0 + d->c1) || d->wld % 64 != 0) return RDEIC_EINVAL;
  if (d->out_mode < 0 || d->out_mode > 2) return RDEIC_EINVAL;
  if (d->out_mode == 1 && (d->cout % 4 != 0)) return RDEIC_EINVAL;
  if (d->out_mode == 2 && (d->dtype != 1 || d->cout % 8 || d->res || d->emb || d->act || d->out_f32 || d->gn_ab ||
                           d->batch > 1 || d->out_ld % 4 || ((uintptr_t)d->out) % 8))
    return RDEIC_EINVAL;
  if (!al16(d->weight)) return RDEIC_EINVAL;
  return RDEIC_OK;
}

bool vec_ok(const rdeic_conv_desc* d) {
  const int epc = d->dtype == 1 ? 8 : 4;
  bool vec = (d->c0 % epc == 0) && (d->ld0 % epc == 0) && al16(d->in0);
  if (d->c1) vec = vec && (d->c1 % epc == 0) && (d->ld1 % epc == 0) && al16(d->in1);
  return vec;
}

// ---- image groups and row bands ----
long image_span(const rdeic_conv_desc* d) {
  const long in = (long)d->h * in_row_bytes(d), out = (long)d->ho * out_row_bytes(d);
  return in > out ? in : out;
}

int band_rows(const rdeic_conv_desc* d, int row_tile) {
  if (d->h <= 0 || d->w <= 0 || d->ho <= 0 || d->wo <= 0 || d->ld0 <= 0 || d->out_ld <= 0) return 0;
  const long lim = g_launch_limit;
  if (image_span(d) <= lim) return d->ho;
  const int kh = d->kh > 0 ? d->kh : 1, stride = d->stride > 0 ? d->stride : 1;
  long step = row_tile > 1 ? row_tile : 1;
  if (d->up2) step = lcm_l(step, 2);  // a band is whole source rows
  if (d->gn_part) {                   // whole 64-row statistic blocks (up2: of each phase's source rows)
    const long q = d->up2 ? 256 : 64;
    step = lcm_l(step, q / gcd_l(d->wo, q));
  }
  // a band of r output rows reaches at most (r - 1) * stride + kh stored input rows (up2, 3x3: r / 2 + 2)
  const long in_rows = lim / in_row_bytes(d);
  long r = d->up2 ? 2 * (in_rows - 2) : (in_rows - kh) / stride + 1;
  if (in_rows < (d->up2 ? 3 : kh)) r = 0;
  const long by_out = lim / out_row_bytes(d);
  if (by_out < r) r = by_out;
  r = r / step * step;
  if (r < step) return 0;
  return (int)(r < d->ho ? r : d->ho);  // full bands from row 0, the last one shorter
}

Band band_at(const rdeic_conv_desc* d, int r0, int rows) {
  Band b;
  b.r0 = r0;
  b.rows = d->ho - r0 < rows ? d->ho - r0 : rows;
  if (d->up2) {  // the phase launch: source rows [r0 / 2, (r0 + rows) / 2) and one row above and below
    const int s0 = r0 / 2, ns = b.rows / 2;
    b.i0 = s0 > 0 ? s0 - 1 : 0;
    b.pad_t = 1 - (s0 - b.i0);
    const int i1 = s0 + ns + 1 < d->h ? s0 + ns + 1 : d->h;
    b.h = i1 - b.i0;
    return b;
  }
  const int top = r0 * d->stride - d->pad_t;  // input row of the band's first tap row
  b.i0 = top > 0 ? top : 0;
  b.pad_t = b.i0 - top;
  const int end = (r0 + b.rows - 1) * d->stride - d->pad_t + d->kh;
  b.h = (end < d->h ? end : d->h) - b.i0;
  return b;
}

int up2_phase_group(const rdeic_conv_desc* d) {
  const long ipix = (long)d->h * d->w;
  const long per_in = ipix * d->ld0 * 2, per_out = 4 * ipix * d->out_ld * 2;
  const long per = per_in > per_out ? per_in : per_out;
  const long lim = g_launch_limit;
  if (d->n <= 0 || per <= 0 || per > lim) return 0;
  long g = lim / per;
  if (g > d->n) g = d->n;
  const long groups = (d->n + g - 1) / g;
  return (int)((d->n + groups - 1) / groups);
}

Slice slice_at(const rdeic_conv_desc* d, const Plan& p, int k) {
  const int bands = cdiv_i(d->ho, p.rows);
  Slice s;
  s.i0 = (k / bands) * p.images;
  s.r0 = (k % bands) * p.rows;
  s.d = *d;
  rdeic_conv_desc& e = s.d;
  e.n = d->n - s.i0 < p.images ? d->n - s.i0 : p.images;
  long irow = 0;  // first stored input row of the slice's window
  if (p.rows < d->ho) {
    const Band b = band_at(d, s.r0, p.rows);
    e.h = b.h; e.ho = b.rows; e.pad_t = b.pad_t;
    irow = b.i0;
  }
  const long ipix = ((long)s.i0 * d->h + irow) * d->w;        // first input pixel
  const long opix = ((long)s.i0 * d->ho + s.r0) * d->wo;      // first output pixel (before a pixel shuffle)
  const long spix = d->out_mode == 1 ? 4 * opix : opix;       // ... of the stored output / residual
  e.in0 = (const char*)d->in0 + ipix * d->ld0 * esize(d);
  e.in1 = d->in1 ? (const char*)d->in1 + ipix * d->ld1 * esize(d) : nullptr;
  e.out = (char*)d->out + spix * d->out_ld * osize(d);
  e.res = d->res ? (const char*)d->res + spix * d->res_ld * osize(d) : nullptr;
  e.emb = d->emb ? d->emb + (long)s.i0 * d->emb_ld : nullptr;
  e.ln_rows = d->ln_rows ? d->ln_rows + 2 * opix : nullptr;
  e.gn_ab = d->gn_ab ? d->gn_ab + (long)s.i0 * (d->c0 + d->c1) * 2 : nullptr;
  s.gn_row0 = opix;
  return s;
}

// ---- per-kernel eligibility of one launch ----
bool dma_ok(const rdeic_conv_desc* d, unsigned& b0, unsigned& b1, unsigned& bw) {
  if (d->dtype != 1 || d->gn_ab || (d->c0 % 64) || (d->c1 % 64) || (d->ld0 % 8) || !al16(d->in0)) return false;
  if (d->c1 && ((d->ld1 % 8) || !al16(d->in1))) return false;
  if (d->wld % 64 || (d->kh * d->kw * (d->c0 + d->c1)) % 64) return false;
  const int batch = batch_of(d);
  const long pix = (long)d->n * d->h * d->w;
  const long e0 = ((pix - 1) * d->ld0 + d->c0) * 2 + (batch - 1) * d->in_bs * 2;
  const long e1 = d->c1 ? ((pix - 1) * d->ld1 + d->c1) * 2 : 16;
  const long ew = (long)d->cout * d->wld * 2 + (batch - 1) * d->w_bs * 2;
  if (e0 > g_launch_limit || e1 > g_launch_limit || ew >= (1l << 31)) return false;
  if (batch > 1 && (d->in_bs % 8 || d->w_bs % 8)) return false;
  // batched operands are addressed from the per-z base: the descriptor covers one slice
  b0 = (unsigned)(((pix - 1) * d->ld0 + d->c0) * 2);
  b1 = (unsigned)e1;
  bw = (unsigned)((long)d->cout * d->wld * 2);
  return true;
}

bool halo_ok(const rdeic_conv_desc* d) {
  return d->dtype == 1 && is_3x3_same(d) && d->c0 % 32 == 0 && d->c0 <= HALO_AB_MAX && d->cout % HALO_BN == 0 &&
         d->h % HALO_TR == 0 && d->w % HALO_TC == 0 && batch_of(d) == 1 && d->out_mode == 0 && d->ld0 % 8 == 0 &&
         al16(d->in0) && d->wld % 64 == 0 && epi_vec_ok(*d) && g_epi_vec;
}

bool halo8_form(const rdeic_conv_desc* d) {
  return g_halo8 && !d->out_f32 && !d->emb && d->act == 0 && d->h % HALO8_TR == 0;
}

bool up2_phases_ok(const rdeic_conv_desc* d, long phase_stride) {
  if (!d || !d->in0 || !d->weight || !d->out || d->n <= 0 || d->h <= 0 || d->w <= 0 || d->cout <= 0) return false;
  if (d->dtype != 1 || d->out_f32 || !d->up2 || d->kh != 3 || d->kw != 3 || d->stride != 1 || d->pad_t != 1 ||
      d->pad_l != 1 || d->ho != 2 * d->h || d->wo != 2 * d->w)
    return false;
  if (d->c1 || d->in1 || d->c0 <= 0 || d->c0 % 64 || d->out_mode != 0 || d->batch > 1) return false;
  if (d->gn_ab || d->emb || d->res || d->ln_rows || d->ln_colsum) return false;
  if (d->wld != 4 * d->c0 || phase_stride < (long)d->cout * d->wld || phase_stride % 8) return false;
  if (d->ld0 < d->c0 || d->ld0 % 8 || !al16(d->in0) || !al16(d->weight)) return false;
  if (d->cout % 8 || d->out_ld < d->cout || d->out_ld % 8 || !al16(d->out)) return false;
  if ((long)d->cout * d->wld * 2 >= (1l << 31)) return false;
  return up2_phase_group(d) > 0 || band_rows(d, 1) > 0;
}

rdeic_conv_desc up2_phase_desc(const rdeic_conv_desc& s) {
  rdeic_conv_desc e = s;  // one phase: the 2x2 conv over the raw input, h x w GEMM rows per image
  e.up2 = 0; e.kh = 2; e.kw = 2; e.stride = 1; e.pad_l = 1; e.ho = s.ho / 2; e.wo = s.w;
  return e;
}

// ---- plans ----
namespace {
void set_launches(const rdeic_conv_desc* d, Plan& p) {
  if (p.images > d->n) p.images = d->n;
  p.launches = cdiv_i(d->n, p.images) * cdiv_i(d->ho, p.rows);
}

// One launch of the DMA kernel takes this (sub-)descriptor: what make_args + dma_ok accept.
bool dma_launch_ok(const rdeic_conv_desc* d) {
  unsigned b0, b1, bw;
  return validate_desc(d) == RDEIC_OK && vec_ok(d) && dma_ok(d, b0, b1, bw);
}

// The LDS-DMA plan: one launch where it fits, else the largest image groups that fit, else row bands of each
// image (out_mode 0, batch 1, no upsample). Every slice is checked before the plan is returned.
bool plan_dma(const rdeic_conv_desc* d, Plan& p) {
  unsigned b0, b1, bw;
  const bool whole = dma_ok(d, b0, b1, bw);
  const long lim = g_launch_limit, per = image_span(d);
  p.images = d->n; p.rows = d->ho; p.launches = 1;
  if (whole && (d->batch > 1 || per * d->n <= lim)) return true;
  if (d->batch > 1) return false;
  if (per <= lim && d->n > 1) {
    p.images = (int)(lim / per);
  } else {
    const int rows = (per > lim && d->out_mode == 0 && !d->up2 && d->dtype == 1) ? band_rows(d, 1) : 0;
    // Kept as it was: one image past the launch limit for which band_rows has no plan (0, or ho) still runs as
    // ONE launch when dma_ok holds for the whole launch; dma_ok bounds the input spans only.
    if (rows <= 0 || rows >= d->ho) return whole;
    p.images = 1; p.rows = rows;
  }
  set_launches(d, p);
  for (int k = 0; k < p.launches; ++k) {
    const Slice s = slice_at(d, p, k);
    if (!dma_launch_ok(&s.d)) return false;
  }
  return true;
}

// The halo / narrow plan: the largest image groups that fit, or row bands (multiples of row_tile) of each image.
// band_rows bounds every band's input, output and residual span by construction.
bool plan_rows(const rdeic_conv_desc* d, int row_tile, Plan& p) {
  const long lim = g_launch_limit, per = image_span(d);
  p.images = 1; p.rows = d->ho;
  if (per <= lim) {
    const long g = lim / per;
    p.images = g < d->n ? (int)g : d->n;
  } else {
    p.rows = band_rows(d, row_tile);
    if (p.rows <= 0) return false;
  }
  set_launches(d, p);
  return true;
}

// what both edge kernels need (conv_edge.hip)
bool edge_common(const rdeic_conv_desc* d) {
  return g_edge && d->dtype == 1 && is_3x3_same(d) && batch_of(d) == 1 && d->out_mode == 0 && d->ld0 % 8 == 0 &&
         al16(d->in0) && al16(d->weight);
}
// conv_in: 8 input channels, bias only, bf16 output; 16 bytes per pixel, so no bands: an input past the kernel's
// 32-bit descriptor takes the general path
bool edge_in8_ok(const rdeic_conv_desc* d) {
  return edge_common(d) && d->c0 == 8 && !d->gn_ab && d->wld >= 128 && d->cout % 32 == 0 && d->cout <= 128 &&
         d->w % 64 == 0 && !d->emb && !d->act && !d->res && !d->out_f32 && !d->ln_rows && d->out_ld % 8 == 0 &&
         al16(d->out) && (long)d->n * d->ho * d->wo * d->ld0 * 2 <= g_launch_limit;
}
// norm -> (SiLU) -> conv to <= 16 channels (table + weights in LDS beside the halo)
bool edge_narrow_ok(const rdeic_conv_desc* d) {
  const long lds = NARROW_LDS + (long)d->c0 * 8 + (long)d->cout * 9 * d->c0 * 2;
  return edge_common(d) && d->gn_ab && d->cout <= 16 && d->c0 % 32 == 0 && d->h % NARROW_TR == 0 &&
         d->w % NARROW_TC == 0 && lds <= 160 * 1024 && !d->gn_part && !d->emb && al16(d->gn_ab);
}
bool smallc_ok(const rdeic_conv_desc* d) {
  return d->dtype == 1 && d->cout <= 4 && d->c0 % 32 == 0 && is_3x3_same(d) && d->out_mode == 0 &&
         batch_of(d) == 1 && g_conv_path != 0;
}
}  // namespace

int plan_conv(const rdeic_conv_desc* d, int tile, bool caller_materializes, Plan& p) {
  const int rc = validate_desc(d);
  if (rc != RDEIC_OK) return rc;
  if (d->gn_part &&
      (d->gn_hw <= 0 || d->gn_hw % 64 || d->batch > 1 || d->out_mode != 0 || (long)d->n * d->ho * d->wo % d->gn_hw))
    return RDEIC_EINVAL;
  const bool vec = vec_ok(d);
  p.images = d->n; p.rows = d->ho; p.launches = 1;
  // the VAE edge convs take their shapes whatever the tile
  if (edge_in8_ok(d)) { p.route = RDEIC_ROUTE_EDGE_IN8; return RDEIC_OK; }
  if (edge_narrow_ok(d) && plan_rows(d, NARROW_TR, p)) { p.route = RDEIC_ROUTE_EDGE_NARROW; return RDEIC_OK; }
  if (d->out_mode == 2) {  // fused GEGLU exists in the LDS-DMA kernel's vector epilogue only (option 5 does not gate it)
    p.route = RDEIC_ROUTE_DMA;
    return vec && plan_dma(d, p) ? RDEIC_OK : RDEIC_EINVAL;
  }
  // the big-tile path: bf16, 16-byte gathers, more than 32 output channels
  const bool big = d->dtype == 1 && vec && d->cout > 32 && g_conv_path != 0;
  // Kept as it was: a call with an explicit tile (rdeic_conv2d_tile, tile >= -1) keeps a conv WITHOUT a GroupNorm
  // input on the big-tile path even when option 6 is 2 (halo for every eligible conv).
  const bool halo_wanted = d->gn_ab ? (g_halo != 0 && d->cout <= HALO_GN_MAX_COUT) : (g_halo == 2 && !(big && tile != -2));
  if (vec && halo_wanted && halo_ok(d) && (long)d->cout * d->wld * 2 < (1l << 31) &&
      plan_rows(d, halo8_form(d) ? HALO8_TR : HALO_TR, p)) {
    p.route = RDEIC_ROUTE_HALO;
    return RDEIC_OK;
  }
  p.images = d->n; p.rows = d->ho; p.launches = 1;
  // No fused-GroupNorm kernel took it. Where the descriptor would run on the big-tile path without gn_ab, and for
  // the large tiny-cout convs (the VAE's conv_out past the narrow kernel's shapes), the caller applies the
  // GroupNorm first: the direct kernels redo the affine (+ SiLU) for every tap. Only rdeic_conv2d_plan asks with
  // caller_materializes; the dispatch never sees this route and runs such a descriptor on the rungs below.
  if (d->gn_ab && caller_materializes && g_conv_path != 0 && d->dtype == 1 && vec &&
      (d->cout > 32 || (d->cout <= 4 && (long)d->n * d->h * d->w >= MATERIALIZE_SMALLC_PIX))) {
    p.route = RDEIC_ROUTE_MATERIALIZE;
    return RDEIC_OK;
  }
  if (vec && smallc_ok(d)) { p.route = RDEIC_ROUTE_SMALLC; return RDEIC_OK; }
  if (big && !d->gn_ab) {
    // Kept as it was: an explicit LDS-DMA tile (>= 20) runs the LDS-DMA kernel even with option 5 at 0
    // (tools/dma_bench.py and ops.FORCE_TILE rely on it); tiles -1 .. 19 never do.
    const bool try_dma = tile == -2 ? g_dma != 0 : tile >= 20;
    if (try_dma && plan_dma(d, p)) { p.route = RDEIC_ROUTE_DMA; return RDEIC_OK; }
    p.images = d->n; p.rows = d->ho; p.launches = 1;
    p.route = RDEIC_ROUTE_TILE;
    return RDEIC_OK;
  }
  p.route = RDEIC_ROUTE_DIRECT;
  return RDEIC_OK;
}

bool plan_up2_phases(const rdeic_conv_desc* d, long phase_stride, Plan& p) {
  if (!up2_phases_ok(d, phase_stride)) return false;
  p.route = RDEIC_ROUTE_DMA;
  p.images = up2_phase_group(d);
  p.rows = d->ho;
  if (p.images == 0) {  // one image is past the launch limit: row bands of each image (band_at: source-row windows)
    p.images = 1;
    p.rows = band_rows(d, 1);
    if (p.rows <= 0) return false;
  }
  set_launches(d, p);
  for (int k = 0; k < p.launches; ++k) {
    const rdeic_conv_desc e = up2_phase_desc(slice_at(d, p, k).d);
    if (!dma_launch_ok(&e)) return false;
  }
  return true;
}

}  // namespace rdeic_conv

using namespace rdeic_conv;

extern "C" int rdeic_conv2d_plan(const rdeic_conv_desc* d, int32_t tile, rdeic_conv_plan* plan) {
  if (!plan) return RDEIC_EINVAL;
  Plan p;
  const int rc = plan_conv(d, tile, true, p);
  if (rc != RDEIC_OK) return rc;
  plan->route = p.route; plan->images = p.images; plan->rows = p.rows; plan->launches = p.launches;
  return RDEIC_OK;
}

// Images per launch of rdeic_conv2d_up2_phases for this descriptor.
extern "C" int rdeic_conv2d_up2_group(const rdeic_conv_desc* d) { return d ? up2_phase_group(d) : 0; }

// Output rows per band of this descriptor's image under the launch limit.
extern "C" int rdeic_conv2d_band_rows(const rdeic_conv_desc* d, int32_t row_tile) { return d ? band_rows(d, row_tile) : 0; }

extern "C" int rdeic_set_conv_path(int32_t path) {
  const int prev = g_conv_path;
  g_conv_path = path;
  return prev;
}

extern int rdeic_g_attn64;
extern int rdeic_g_attn512;

extern "C" int rdeic_set_conv_option(int32_t key, int32_t value) {
  int* const opt[] = {&g_epi_vec, &rdeic_g_attn64, nullptr, &g_swz,   &g_force_tile, &g_dma,       &g_halo,
                      nullptr,    &rdeic_g_attn512, &g_halo8, &g_edge, &g_up2_phases, &g_launch_limit};
  if (key < 0 || key > 12 || !opt[key]) return RDEIC_EINVAL;
  const int prev = *opt[key];
  *opt[key] = (key == 12 && value <= 0) ? 0x7fffffff : value;
  return prev;
}

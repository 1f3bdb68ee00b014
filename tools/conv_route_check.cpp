// Stand-alone walk of the conv planner (rdeic_amd/csrc/conv_route.cpp) for a host sanitizer run: no GPU, no Python,
// nothing linked but the planner. It plans every descriptor of tests/conv_routes_parent.json plus a set of extremes,
// visits every slice of every plan (bounded per plan) and checks that the slices tile the conv.
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/conv_route_check.cpp rdeic_amd/csrc/conv_route.cpp -o tools/conv_route_check
//   tools/conv_route_check tests/conv_routes_parent.json
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../rdeic_amd/csrc/conv_route.h"

int rdeic_g_attn64 = 1, rdeic_g_attn512 = 2;  // the attention switches rdeic_set_conv_option also serves

using namespace rdeic_conv;

static char* const A = (char*)0x10000000;  // an aligned address; the planner never reads through it
static long g_plans = 0, g_slices = 0;

static rdeic_conv_desc desc(int k, int c, int cout, int n, int h, int w, int bits) {
  rdeic_conv_desc d = {};
  const bool concat = bits & 1, res = bits & 2, up2 = bits & 4, of32 = bits & 8, emb = bits & 16, sliced = bits & 32;
  d.c0 = concat ? c / 2 : c; d.ld0 = d.c0; d.in0 = A;
  if (concat) { d.c1 = c - d.c0; d.ld1 = d.c1; d.in1 = A + 0x10000000; }
  d.n = n; d.h = h; d.w = w; d.up2 = up2;
  d.weight = A + 0x20000000; d.wld = (k * k * c + 63) / 64 * 64;
  d.cout = cout; d.kh = d.kw = k; d.stride = 1; d.pad_t = d.pad_l = k / 2;
  d.ho = up2 ? 2 * h : h; d.wo = up2 ? 2 * w : w;
  d.gn_ab = (const float*)(A + 0x30000000); d.gn_silu = 1;
  if (emb) { d.emb = (const float*)(A + 0x40000000); d.emb_ld = cout; }
  d.out = A + 0x50000000; d.out_ld = sliced ? 2 * cout : cout;
  if (res) { d.res = A + 0x60000000; d.res_ld = cout; }
  d.dtype = 1; d.out_f32 = of32; d.batch = 1;
  return d;
}

// plan d for both entry points and walk the slices: consecutive, inside the conv, covering it exactly
static void walk(const rdeic_conv_desc& d) {
  for (int tile : {-2, -1, 3, 25}) {
    Plan p;
    if (plan_conv(&d, tile, true, p) != RDEIC_OK) continue;
    ++g_plans;
    if (p.images <= 0 || p.rows <= 0 || p.launches <= 0) { std::printf("empty plan\n"); std::exit(1); }
    long cells = 0;
    // every slice of a small plan; of a huge one (launch limit 1) the first and last 2048
    for (int k = 0; k < p.launches; ++k) {
      if (p.launches > 4096 && k == 2048) k = p.launches - 2048;
      const Slice s = slice_at(&d, p, k);
      if (s.i0 < 0 || s.i0 + s.d.n > d.n || s.r0 < 0 || s.r0 + s.d.ho > d.ho || s.d.n <= 0 || s.d.ho <= 0 ||
          s.d.h <= 0 || s.d.h > d.h) {
        std::printf("slice %d of %d outside the conv\n", k, p.launches);
        std::exit(1);
      }
      cells += (long)s.d.n * s.d.ho;
      ++g_slices;
    }
    if (p.launches <= 4096 && cells != (long)d.n * d.ho) { std::printf("slices do not tile the conv\n"); std::exit(1); }
  }
  Plan p;
  if (d.up2 && plan_up2_phases(&d, (long)d.cout * d.wld, p))
    for (int k = 0; k < p.launches; ++k) { (void)up2_phase_desc(slice_at(&d, p, k).d); ++g_slices; }
  (void)band_rows(&d, 1); (void)band_rows(&d, 4); (void)band_rows(&d, 8); (void)up2_phase_group(&d);
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: conv_route_check tests/conv_routes_parent.json\n"); return 2; }
  std::stringstream ss;
  ss << std::ifstream(argv[1]).rdbuf();
  const std::string js = ss.str();
  size_t at = js.find("\"rows\":[");
  if (at == std::string::npos) { std::printf("no rows\n"); return 2; }
  at += 8;
  // rows: [k, c, cout, n, h, w, flags, limit, halo, narrow, materialize] of integers
  while (at < js.size() && js[at] == '[') {
    std::vector<long> v;
    const char* q = js.c_str() + at + 1;
    char* e = nullptr;
    for (;;) {
      v.push_back(std::strtol(q, &e, 10));
      if (*e != ',') break;
      q = e + 1;
    }
    at = (size_t)(e - js.c_str()) + 1;  // past ']'
    if (at < js.size() && js[at] == ',') ++at;
    if (v.size() != 11) { std::printf("bad row\n"); return 2; }
    rdeic_set_conv_option(12, (int)v[7]);
    walk(desc((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6]));
  }
  const long table = g_plans;
  // extremes, at the default limit, at lowered ones and at a limit of one byte
  for (int limit : {0, 1 << 30, 1 << 20, 4097, 1}) {
    rdeic_set_conv_option(12, limit);
    for (int gn : {0, 1})
      for (int bits : {0, 2, 4, 8 | 16, 1}) {
        rdeic_conv_desc e[] = {desc(3, 128, 128, 16, 1024, 1024, bits), desc(3, 128, 128, 1, 4096, 4096, bits),
                               desc(1, 128, 3, 1, 4096, 4096, bits),    desc(3, 1280, 1280, 64, 2048, 2048, bits),
                               desc(1, 64, 1024, 1, 8, 1024, bits),     desc(3, 8, 128, 4, 512, 512, bits)};
        for (rdeic_conv_desc& d : e) {  // the fourth: n * h * w * ld past 2^32 (and 2^38 bytes)
          if (!gn) d.gn_ab = nullptr;
          d.gn_part = (float*)(A + 0x70000000); d.gn_hw = d.ho * d.wo;
          walk(d);
          d.gn_part = nullptr;
          walk(d);
        }
      }
  }
  rdeic_set_conv_option(12, 0);
  std::printf("conv_route_check: %ld table plans, %ld extreme plans, %ld slices walked: ok\n", table, g_plans - table,
              g_slices);
  return 0;
}

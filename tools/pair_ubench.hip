// Pairing probe (diagnostics, not part of the product): does a SIMD issue the
// 2-cycle class (v_xor_b32) at 2 cycles only when its waves offer it in the
// same turn, and can a barrier or a priority change in front of every fast
// group of the compression make them do so?
//
// Bodies (80 VALU instructions per iteration):
//   A, L, X   pure v_lshl_add_u64 / v_alignbit_b32 / v_xor_b32 (mix_bodies.h)
//   A8X8      (8 A | 8 X) x 5, the instructions of MIX_A8X8
//   A16X16    16 A | 16 X | 16 A | 16 X | 16 A, the instructions of MIX_A16X16
//   G         one step-major half round with its real dependencies, the group
//             pattern of g4 (blake2b_dev.hpp):
//             8S | 8F | 4S | 8F | 16S | 8F | 12S | 8F | 8S
// The mixed bodies are built from pieces here so that a hook can stand in
// front of (and behind) every fast group.
//
// Arms:
//   free      no hook                                   (a at 256 threads)
//   bar/fast  s_barrier in front of every fast group    (b at 512, c at 1024)
//   bar/body  one s_barrier per body                    (d)
//   prio      s_setprio 1 across every fast group       (e)
// at 256-, 512- and 1024-thread workgroups and 2 or 4 waves per SIMD.  The
// occupancy is set by the register count (a clobber of v255 or v127: 512
// VGPRs per SIMD / 256 or 128), the grid is exactly one resident round, and
// every wave stamps s_memtime around its loop, so the cycles are the chip's
// own and do not depend on the clock it holds.  Every wave also records its
// HW_ID: the log shows how many waves each SIMD really held and where the
// waves of one workgroup sat.  A SIMD's cost per instruction is the longest
// loop among its waves over the instructions of all of them (free-running
// waves do not share a SIMD evenly: the oldest finishes first).
//
// Every wave of a workgroup runs the same `iters` (a kernel argument)
// iterations of the same straight-line body, so all of them reach every
// barrier.
//
//   hipcc -O3 --offload-arch=gfx950 -Itools tools/pair_ubench.hip -o build/pair_ubench
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <vector>

#include "mix_bodies.h"

#define CK(x)                                                                    \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) {                                                      \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

#define CLOBBERS "v10","v11","v12","v13","v14","v15","v16","v17","v18","v19","v20","v21","v22","v23","v24","v25","v26","v27","v28","v29","v30","v31","v32","v33","v34","v35","v36","v37","v38","v39","v40","v41","v42","v43","v44","v45","v46","v47","v48","v49","v50","v51","v52","v53","v54","v55","v56","v57","v58","v59","v60","v61"

// ---- independent pieces (the register streams of mix_bodies.h) -------------
#define P_A(l, h) "v_lshl_add_u64 v[" #l ":" #h "], v[" #l ":" #h "], 0, v[58:59]\n"
#define P_L(r) "v_alignbit_b32 v" #r ", v" #r ", v59, 7\n"
#define P_X(r) "v_xor_b32 v" #r ", v" #r ", v60\n"
#define P_A8 P_A(10, 11) P_A(12, 13) P_A(14, 15) P_A(16, 17) P_A(18, 19) P_A(20, 21) P_A(22, 23) P_A(24, 25)
#define P_X8a P_X(42) P_X(43) P_X(44) P_X(45) P_X(46) P_X(47) P_X(48) P_X(49)
#define P_X8b P_X(50) P_X(51) P_X(52) P_X(53) P_X(54) P_X(55) P_X(56) P_X(57)

#define BODY_A8X8(PRE, POST)                                                      \
  P_A8 PRE P_X8a POST P_A8 PRE P_X8b POST P_A8 PRE P_X8a POST P_A8 PRE P_X8b POST \
  P_A8 PRE P_X8a POST
#define BODY_A16X16(PRE, POST)                                                    \
  P_A8 P_A8 PRE P_X8a P_X8b POST P_A8 P_A8 PRE P_X8a P_X8b POST P_A8 P_A8
#define BODY_PA(PRE, POST) PRE MIX_A POST
#define BODY_PL(PRE, POST) PRE MIX_L POST
#define BODY_PX(PRE, POST) PRE MIX_X POST

// ---- the step-major half round ---------------------------------------------
// Column k: a, b, c, d, t (the rotr-32 result), u (xor scratch); x = v[58:59],
// y = v[60:61].  The register assignment of ASM_HALF_STEP (asm_g_bodies.h).
#define COLS(M)                                               \
  M(10, 11, 18, 19, 26, 27, 34, 35, 42, 43, 44, 45)           \
  M(12, 13, 20, 21, 28, 29, 36, 37, 46, 47, 48, 49)           \
  M(14, 15, 22, 23, 30, 31, 38, 39, 50, 51, 52, 53)           \
  M(16, 17, 24, 25, 32, 33, 40, 41, 54, 55, 56, 57)
#define G_AX(al, ah, bl, bh, cl, ch, dl, dh, t0, t1, u0, u1) \
  "v_lshl_add_u64 v[" #al ":" #ah "], v[" #al ":" #ah "], 0, v[58:59]\n"
#define G_AY(al, ah, bl, bh, cl, ch, dl, dh, t0, t1, u0, u1) \
  "v_lshl_add_u64 v[" #al ":" #ah "], v[" #al ":" #ah "], 0, v[60:61]\n"
#define G_AB(al, ah, bl, bh, cl, ch, dl, dh, t0, t1, u0, u1) \
  "v_lshl_add_u64 v[" #al ":" #ah "], v[" #al ":" #ah "], 0, v[" #bl ":" #bh "]\n"
#define G_DA32(al, ah, bl, bh, cl, ch, dl, dh, t0, t1, u0, u1) \
  "v_xor_b32 v" #t0 ", v" #dh ", v" #ah "\nv_xor_b32 v" #t1 ", v" #dl ", v" #al "\n"
#define G_CT(al, ah, bl, bh, cl, ch, dl, dh, t0, t1, u0, u1) \
  "v_lshl_add_u64 v[" #cl ":" #ch "], v[" #cl ":" #ch "], 0, v[" #t0 ":" #t1 "]\n"
#define G_BC(al, ah, bl, bh, cl, ch, dl, dh, t0, t1, u0, u1) \
  "v_xor_b32 v" #u0 ", v" #bl ", v" #cl "\nv_xor_b32 v" #u1 ", v" #bh ", v" #ch "\n"
#define G_R24(al, ah, bl, bh, cl, ch, dl, dh, t0, t1, u0, u1) \
  "v_alignbit_b32 v" #bl ", v" #u1 ", v" #u0 ", 24\nv_alignbit_b32 v" #bh ", v" #u0 ", v" #u1 ", 24\n"
#define G_TA(al, ah, bl, bh, cl, ch, dl, dh, t0, t1, u0, u1) \
  "v_xor_b32 v" #u0 ", v" #t0 ", v" #al "\nv_xor_b32 v" #u1 ", v" #t1 ", v" #ah "\n"
#define G_R16(al, ah, bl, bh, cl, ch, dl, dh, t0, t1, u0, u1) \
  "v_alignbit_b32 v" #dl ", v" #u1 ", v" #u0 ", 16\nv_alignbit_b32 v" #dh ", v" #u0 ", v" #u1 ", 16\n"
#define G_CD(al, ah, bl, bh, cl, ch, dl, dh, t0, t1, u0, u1) \
  "v_lshl_add_u64 v[" #cl ":" #ch "], v[" #cl ":" #ch "], 0, v[" #dl ":" #dh "]\n"
#define G_R63(al, ah, bl, bh, cl, ch, dl, dh, t0, t1, u0, u1) \
  "v_alignbit_b32 v" #bl ", v" #u0 ", v" #u1 ", 31\nv_alignbit_b32 v" #bh ", v" #u1 ", v" #u0 ", 31\n"
#define BODY_G(PRE, POST)                                          \
  COLS(G_AX) COLS(G_AB) PRE COLS(G_DA32) POST COLS(G_CT)           \
  PRE COLS(G_BC) POST COLS(G_R24) COLS(G_AY) COLS(G_AB)            \
  PRE COLS(G_TA) POST COLS(G_R16) COLS(G_CD)                       \
  PRE COLS(G_BC) POST COLS(G_R63)

enum { kFree = 0, kBarFast = 1, kBarBody = 2, kPrio = 3 };

#define RUN_BODY(B)                                                                       \
  do {                                                                                    \
    if constexpr (ARM == kFree) asm volatile(B("", "")::: CLOBBERS);                      \
    if constexpr (ARM == kBarFast) asm volatile(B("s_barrier\n", "")::: CLOBBERS);        \
    if constexpr (ARM == kBarBody) asm volatile("s_barrier\n" B("", "")::: CLOBBERS);     \
    if constexpr (ARM == kPrio) asm volatile(B("s_setprio 1\n", "s_setprio 0\n")::: CLOBBERS); \
  } while (0)

// dbg[4 w .. 4 w + 3] of wave w = HW_ID | XCC_ID << 32, shader cycles of the
// loop, 100 MHz ticks of the loop, a value that keeps the loop alive.
template <int BODY, int ARM, int WG, int WPS>
__global__ __launch_bounds__(WG) void k_pair(uint64_t* dbg, uint32_t max_waves, int iters) {
  // the register count sets the occupancy: 512 / 256 = 2 or 512 / 128 = 4 waves per SIMD
  if constexpr (WPS == 2)
    asm volatile("" ::: "v255");
  else
    asm volatile("" ::: "v127");
  uint32_t hwid, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
  for (int i = 0; i < iters; ++i) {
    if constexpr (BODY == 0) RUN_BODY(BODY_PA);
    if constexpr (BODY == 1) RUN_BODY(BODY_PL);
    if constexpr (BODY == 2) RUN_BODY(BODY_PX);
    if constexpr (BODY == 3) RUN_BODY(BODY_A8X8);
    if constexpr (BODY == 4) RUN_BODY(BODY_A16X16);
    if constexpr (BODY == 5) RUN_BODY(BODY_G);
  }
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  const uint64_t r1 = __builtin_amdgcn_s_memrealtime();
  uint32_t v;
  asm volatile("v_mov_b32 %0, v10" : "=v"(v));
  const uint32_t w = blockIdx.x * (WG / 64) + threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0 && w < max_waves) {
    dbg[4 * (uint64_t)w + 0] = hwid | (uint64_t)(xcc & 0xf) << 32;
    dbg[4 * (uint64_t)w + 1] = t1 - t0;
    dbg[4 * (uint64_t)w + 2] = r1 - r0;
    dbg[4 * (uint64_t)w + 3] = v;
  }
}

typedef void (*Kf)(uint64_t*, uint32_t, int);

struct Row {
  const char* arm;
  int armk, wg, wps;
  Kf k[6];
};
#define ROW(NAME, ARM, WG, WPS)                                                              \
  {NAME, ARM, WG, WPS,                                                                       \
   {k_pair<0, ARM, WG, WPS>, k_pair<1, ARM, WG, WPS>, k_pair<2, ARM, WG, WPS>,               \
    k_pair<3, ARM, WG, WPS>, k_pair<4, ARM, WG, WPS>, k_pair<5, ARM, WG, WPS>}}

static const char* kBodies[6] = {"A", "L", "X", "A8X8", "A16X16", "G"};
// adds, funnel shifts, xors of each body
static const int kMix[6][3] = {{80, 0, 0}, {0, 80, 0}, {0, 0, 80}, {40, 0, 40}, {48, 0, 32}, {24, 24, 32}};

// SIMD of a wave: XCC, SE, SH, CU and SIMD fields of HW_ID (gfx9 layout:
// wave 3:0, simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13)
static uint64_t simd_key(uint64_t d0) { return (d0 >> 32) << 16 | (d0 & 0xff30u); }

int main() {
  int cus = 0;
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  const uint32_t max_waves = (uint32_t)cus * 16u;
  uint64_t* dbg;
  CK(hipMalloc(&dbg, (size_t)max_waves * 32));
  const Row rows[] = {
      ROW("a free     wg256 ", kFree, 256, 2),  ROW("a free     wg256 ", kFree, 256, 4),
      ROW("  free     wg512 ", kFree, 512, 2),  ROW("  free     wg512 ", kFree, 512, 4),
      ROW("  free     wg1024", kFree, 1024, 4),
      ROW("b bar/fast wg512 ", kBarFast, 512, 2), ROW("b bar/fast wg512 ", kBarFast, 512, 4),
      ROW("c bar/fast wg1024", kBarFast, 1024, 4),
      ROW("d bar/body wg512 ", kBarBody, 512, 2), ROW("d bar/body wg512 ", kBarBody, 512, 4),
      ROW("d bar/body wg1024", kBarBody, 1024, 4),
      ROW("e prio     wg256 ", kPrio, 256, 2),  ROW("e prio     wg256 ", kPrio, 256, 4),
      ROW("e prio     wg1024", kPrio, 1024, 4),
  };
  const int iters = 4096;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<uint64_t> h((size_t)max_waves * 4);
  printf("%d CUs, %d iterations of 80 instructions; cpi = shader cycles (s_memtime) per wave\n"
         "instruction per SIMD, median over the SIMDs; sum = the class-rate sum of the free\n"
         "wg256 run at the same occupancy in the same pass\n", cus, iters);
  for (int pass = 0; pass < 2; ++pass) {
    double pure[5][3] = {};  // [wps][class] from arm a
    double free_cpi[5][6] = {};
    for (const Row& r : rows) {
      const int nwaves = cus * 4 * r.wps;  // one resident round
      const int grid = nwaves / (r.wg / 64);
      for (int b = 0; b < 6; ++b) {
        hipLaunchKernelGGL(r.k[b], dim3(grid), dim3(r.wg), 0, 0, dbg, max_waves, iters);  // warm
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(r.k[b], dim3(grid), dim3(r.wg), 0, 0, dbg, max_waves, iters);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        CK(hipMemcpy(h.data(), dbg, (size_t)nwaves * 32, hipMemcpyDeviceToHost));
        std::vector<double> ghz(nwaves);
        std::map<uint64_t, int> per_simd;
        std::map<uint64_t, double> simd_cyc;  // the longest loop among the SIMD's waves
        for (int w = 0; w < nwaves; ++w) {
          ghz[w] = h[4 * w + 2] ? (double)h[4 * w + 1] / (double)h[4 * w + 2] * 0.1 : 0;
          const uint64_t key = simd_key(h[4 * w]);
          ++per_simd[key];
          simd_cyc[key] = std::max(simd_cyc[key], (double)h[4 * w + 1]);
        }
        std::vector<double> cyc;
        for (auto& kv : simd_cyc) cyc.push_back(kv.second);
        std::sort(cyc.begin(), cyc.end());
        std::sort(ghz.begin(), ghz.end());
        const double cpi = cyc[cyc.size() / 2] / ((double)iters * 80 * r.wps);
        const double cpi_max = cyc.back() / ((double)iters * 80 * r.wps);
        // simd_key assumes the gfx9 HW_ID layout: one resident round fills every SIMD
        if (per_simd.size() != (size_t)cus * 4) {
          fprintf(stderr, "%zu distinct SIMD ids, expected %d: HW_ID layout?\n", per_simd.size(),
                  cus * 4);
          return 1;
        }
        int lo = 1 << 30, hi = 0;
        for (auto& kv : per_simd) {
          lo = std::min(lo, kv.second);
          hi = std::max(hi, kv.second);
        }
        if (r.armk == kFree && r.wg == 256) {
          if (b < 3) pure[r.wps][b] = cpi;
          free_cpi[r.wps][b] = cpi;
        }
        const double* p = pure[r.wps];
        const double sum = (kMix[b][0] * p[0] + kMix[b][1] * p[1] + kMix[b][2] * p[2]) / 80.0;
        const double gap = free_cpi[r.wps][b] - sum;
        printf("%s %d w/SIMD %-6s %7.3f ms  cpi %.3f (slowest SIMD %.3f)  sum %.3f  gap closed %5.1f %%"
               "  %.3f GHz  SIMDs %zu, waves per SIMD %d..%d\n",
               r.arm, r.wps, kBodies[b], ms, cpi, cpi_max, sum,
               gap > 0.01 ? 100.0 * (free_cpi[r.wps][b] - cpi) / gap : 0.0, ghz[nwaves / 2],
               per_simd.size(), lo, hi);
        if (pass == 0 && b == 5) {
          // where the waves of the first two workgroups sat: xcc.se.cu:simd
          const int wpw = r.wg / 64;
          for (int g = 0; g < 2 && g < grid; ++g) {
            printf("    workgroup %d:", g);
            for (int w = g * wpw; w < (g + 1) * wpw; ++w) {
              const uint64_t d = h[4 * w];
              printf(" %u.%u.%u:%u", (unsigned)(d >> 32), (unsigned)(d >> 13 & 7),
                     (unsigned)(d >> 8 & 15), (unsigned)(d >> 4 & 3));
            }
            printf("\n");
          }
        }
        fflush(stdout);
      }
    }
  }
  return 0;
}

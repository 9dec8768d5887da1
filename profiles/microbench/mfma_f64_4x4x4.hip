// mfma_f64_4x4x4.hip -- v_mfma_f64_4x4x4_4b_f64 on gfx950 beside v_mfma_f64_16x16x4_f64, one wave alone on a CU:
//   (1) issue interval (eight independent accumulators) and dependent latency (through C, and through the B operand) of both forms;
//   (2) the block elimination's patterns (block_elim.hpp): panel -> trailing update -> panel on one tile, and the chief's step of the
//       first half (two panels + three updates) and of the second half (one panel + one update), with the panel in either form;
//   (3) the lane layout of the 4x4x4 form: A, B filled with small integers per lane, D printed and compared with
//           D[16 i + 4 b + j] = sum_k A[16 k + 4 b + i] * B[16 k + 4 b + j]          (block b, entry (i, j))
//       -- under that rule a panel's result lies where register 0 of the 16x16x4 product has it, and no lane moves.
//   profiles/microbench/bin/mfma_f64_4x4x4
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double f64x4 __attribute__((ext_vector_type(4)));
#define M16(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0)
#define M4(a, b, c) __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0)
constexpr int kIter = 4096;
enum { kInd16, kDepC16, kInd4, kDepC4, kDepB4, kDepB16, kPair16, kPair4, kFirst16, kFirst4, kSecond16, kSecond4, kModes };

template <bool P4> __device__ __forceinline__ double panel(double w, double x) {
  if (P4) return M4(w, x, 0.0);
  const f64x4 p = M16(w, x, (f64x4{0.0, 0.0, 0.0, 0.0}));
  return p[0];
}
// one tile: panel of register 0 -> update of the tile with the panel's result -> the next panel waits for the update
template <bool P4> __device__ __forceinline__ void pair_loop(double w, f64x4& t) {
  for (int it = 0; it < kIter; ++it) {
    const double p = panel<P4>(w, t[0]);
    t = M16(p, p, t);
  }
}
// the chief's step, columns 0..15: p0, p1 (both need only w), then t00 (what the next step's panels wait for), t01, t11
template <bool P4> __device__ __forceinline__ void first_loop(double w, f64x4& t00, f64x4& t01, f64x4& t11) {
  for (int it = 0; it < kIter; ++it) {
    const double p0 = panel<P4>(w, t00[0]);
    const double p1 = panel<P4>(w, t01[0]);
    t00 = M16(p0, p0, t00);
    t01 = M16(p0, p1, t01);
    t11 = M16(p1, p1, t11);
  }
}

__global__ void rate(double* out, unsigned long long* ticks, int mode, double w) {
  const int lane = threadIdx.x;
  const double a = double(lane & 15) * 1e-3, b = double(lane >> 4) * 1e-3;
  f64x4 t[8];
  double s[8];
  for (int i = 0; i < 8; ++i) { t[i] = f64x4{a, b, a + b, a - b}; s[i] = a + double(i) * b; }
  const unsigned long long t0 = __builtin_readcyclecounter();
  switch (mode) {
    case kInd16:
      for (int it = 0; it < kIter / 8; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = M16(a, b, t[i]);
      }
      break;
    case kDepC16: for (int it = 0; it < kIter; ++it) t[0] = M16(a, b, t[0]); break;
    case kInd4:
      for (int it = 0; it < kIter / 8; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = M4(a, b, s[i]);
      }
      break;
    case kDepC4: for (int it = 0; it < kIter; ++it) s[0] = M4(a, b, s[0]); break;
    case kDepB4: for (int it = 0; it < kIter; ++it) s[0] = M4(w, s[0], 0.0); break;
    case kDepB16: for (int it = 0; it < kIter; ++it) s[0] = panel<false>(w, s[0]); break;
    case kPair16: pair_loop<false>(w, t[0]); break;
    case kPair4: pair_loop<true>(w, t[0]); break;
    case kFirst16: first_loop<false>(w, t[0], t[1], t[2]); break;
    case kFirst4: first_loop<true>(w, t[0], t[1], t[2]); break;
    // (columns 16..31: one panel and one update per step -- the pair, with the chief's name)
    case kSecond16: pair_loop<false>(w, t[2]); break;
    case kSecond4: pair_loop<true>(w, t[2]); break;
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  double sum = 0.0;
  for (int i = 0; i < 8; ++i) sum += t[i][0] + t[i][1] + t[i][2] + t[i][3] + s[i];
  out[lane] = sum;
  if (lane == 0) ticks[0] = t1 - t0;
}

__global__ void layout(const double* A, const double* B, double* D4, double* D16r0) {
  const int lane = threadIdx.x;
  D4[lane] = M4(A[lane], B[lane], 0.0);
  const f64x4 p = M16(A[lane], B[lane], (f64x4{0.0, 0.0, 0.0, 0.0}));
  D16r0[lane] = p[0];
}

int main() {
  double* out; unsigned long long* ticks;
  if (hipMalloc(&out, 64 * 8) != hipSuccess || hipMalloc(&ticks, 8) != hipSuccess) { std::printf("no device\n"); return 1; }
  const char* what[kModes] = {
      "16x16x4, eight independent accumulators (issue interval)", "16x16x4, dependent through C",
      "4x4x4,   eight independent accumulators (issue interval)", "4x4x4,   dependent through C",
      "4x4x4,   dependent through the B operand (panel -> panel)", "16x16x4, register 0 -> B operand (panel -> panel)",
      "pair:   16x16x4 panel -> 16x16x4 update -> panel ...", "pair:   4x4x4 panel   -> 16x16x4 update -> panel ...",
      "chief, columns 0..15:  2 panels (16x16x4) + 3 updates", "chief, columns 0..15:  2 panels (4x4x4)   + 3 updates",
      "chief, columns 16..31: 1 panel (16x16x4) + 1 update", "chief, columns 16..31: 1 panel (4x4x4)   + 1 update"};
  std::printf("one wave alone on a CU, %d iterations per loop; shader clocks (__builtin_readcyclecounter) per iteration, best of 5 launches\n", kIter);
  for (int m = 0; m < kModes; ++m) {
    unsigned long long best = ~0ull;
    for (int rep = 0; rep < 5; ++rep) {
      hipLaunchKernelGGL(rate, dim3(1), dim3(64), 0, 0, out, ticks, m, 1e-3);
      unsigned long long h = 0;
      if (hipMemcpy(&h, ticks, 8, hipMemcpyDeviceToHost) != hipSuccess) { std::printf("launch failed\n"); return 1; }
      if (h < best) best = h;
    }
    std::printf("%-58s %8.1f\n", what[m], double(best) / kIter);
  }
  // ---- layout ----
  double hA[64], hB[64], hD[64], hD16[64], want[64], want16[64];
  for (int l = 0; l < 64; ++l) { hA[l] = double(l + 1); hB[l] = double(100 + 7 * l + (l * l) % 11); }
  for (int i = 0; i < 4; ++i) for (int b = 0; b < 4; ++b) for (int j = 0; j < 4; ++j) {
    double acc = 0.0;
    for (int k = 0; k < 4; ++k) acc += hA[16 * k + 4 * b + i] * hB[16 * k + 4 * b + j];
    want[16 * i + 4 * b + j] = acc;
  }
  // register 0 of the 16x16x4 product of the SAME B with the A operand the elimination uses today (rows 0..3 of A: lanes l16 < 4):
  // D[i][j] at lane 16 i + j = sum_k A[16 k + i] B[16 k + j]
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 16; ++j) {
    double acc = 0.0;
    for (int k = 0; k < 4; ++k) acc += hA[16 * k + i] * hB[16 * k + j];
    want16[16 * i + j] = acc;
  }
  double *dA, *dB, *dD, *dD16;
  hipMalloc(&dA, 512); hipMalloc(&dB, 512); hipMalloc(&dD, 512); hipMalloc(&dD16, 512);
  hipMemcpy(dA, hA, 512, hipMemcpyHostToDevice); hipMemcpy(dB, hB, 512, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(layout, dim3(1), dim3(64), 0, 0, dA, dB, dD, dD16);
  if (hipMemcpy(hD, dD, 512, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hD16, dD16, 512, hipMemcpyDeviceToHost) != hipSuccess) { std::printf("layout launch failed\n"); return 1; }
  int bad = 0, bad16 = 0;
  std::printf("\nlayout: A[lane] = lane + 1, B[lane] = 100 + 7 lane + lane^2 mod 11. D of the 4x4x4 form by lane (rows: lane >> 4), expected in brackets where it differs\n");
  for (int l = 0; l < 64; ++l) {
    if (hD[l] != want[l]) { ++bad; std::printf(" %8.0f[%8.0f]", hD[l], want[l]); } else std::printf(" %8.0f", hD[l]);
    if (l % 16 == 15) std::printf("\n");
    if (hD16[l] != want16[l]) ++bad16;
  }
  std::printf("4x4x4:   D[16 i + 4 b + j] = sum_k A[16 k + 4 b + i] B[16 k + 4 b + j]: %s (%d of 64 lanes differ)\n", bad ? "NO" : "yes", bad);
  std::printf("16x16x4: register 0, D[16 i + j] = sum_k A[16 k + i] B[16 k + j], i < 4:  %s (%d of 64 lanes differ)\n", bad16 ? "NO" : "yes", bad16);
  return bad ? 2 : 0;
}

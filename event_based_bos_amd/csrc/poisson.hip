// poisson.hip -- Poisson integration of a batch of BOS flows (the reference's poisson_reconstruct, src/utils/stat_utils.py:142-199,
// and the uint8 picture of src/visualizer.py:419-435) as four fp64 matrix-core GEMMs per batch.
//
// For a flow [2, H, W] (component 0 = gradx, 1 = grady) and a boundary image Bd (zeros when absent), h = H - 2, w = W - 2:
//   F[i, j] = (gx[i+1, j+1] - gx[i+1, j]) + (gy[i+1, j+1] - gy[i, j+1]) - stencil(Bd)   (differences in the input type, the sum in
//             float64, the 5-point stencil of Bd with its interior zeroed in the boundary's type -- the reference's order)
//   P = S_h^T ((S_h F S_w^T) / D) S_w,  D[i, j] = (2 cos(pi (j+1) / W) - 2) + (2 cos(pi (i+1) / H) - 2)
// with S_N the orthonormal DST-II matrix (scipy's dst(norm="ortho")): S_N[k, n] = c_k 2 sin(pi m / (2N)), m = (k+1)(2n+1) mod 4N,
// c_k = sqrt(1 / (2N)), c_{N-1} = sqrt(1 / (4N)); its inverse (ortho DST-III) is S_N^T.  The result is Bd with its interior
// replaced by P, in the boundary's type.
//
// Launches, all on the caller's stream, no atomics, no split-K:
//   poisson_dst_matrices   S_h, S_h^T, S_w, S_w^T into scratch, zero-padded to hp = roundup(h, 64), wp = roundup(w, 64), so
//                          no GEMM tile needs a mask on a transform operand;
//   poisson_gemm<STEP 0>   T = F S_w^T: ONE tall GEMM over the B hp rows of the batch; F is formed in the prologue from the flow and
//                          the boundary (rows >= h and columns >= w of F read as zero);
//   poisson_gemm<STEP 1>   G = (S_h T) / D per item; the epilogue forms D in registers and writes zero outside h x w;
//   poisson_gemm<STEP 2>   U = S_h^T G per item;
//   poisson_gemm<STEP 3>   P = U S_w, one tall GEMM; the epilogue writes the interior into the output (the boundary's type), copies
//                          the boundary frame and writes each tile's max |P| (frame included) into scratch;
//   poisson_image          (optional) the visualizer's uint8 image, trunc(P / max|P| * 127 + 128) in the output type.
// Every output element is one fixed sequence of MFMAs over K, so an item's bits do not depend on the batch or on the run.
//
// GEMM tile: 64 x 64 per workgroup of four waves, each wave 32 x 32 as 2 x 2 v_mfma_f64_16x16x4_f64 accumulators; K in steps of 16
// through double-buffered LDS (one barrier per step; the next step's global loads are in flight during the MFMAs).
// v_mfma_f64_16x16x4_f64 lane maps: A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15];
// C/D element r of lane l: row (l >> 4) + 4 r, column l & 15.
#pragma clang fp contract(off)

#include "common.h"

namespace ebos {
namespace {

constexpr int kPoTile = 64;            // M and N of a workgroup tile
constexpr int kPoK = 16;               // K per LDS step
constexpr int kPoBlock = 256;          // four waves, 2 x 2 of 32 x 32
constexpr int kPoLd = kPoTile + 16;    // LDS row pitch in doubles: the four k rows a wave reads land on two bank halves
constexpr int kPoImgBlock = 256;
constexpr int kPoImgPix = 4;           // pixels per thread of poisson_image

typedef double po_acc __attribute__((ext_vector_type(4)));

struct PoGeom {
  int h, w, hp, wp, mt, nt;   // interior, padded interior, tiles per item along M (hp / 64) and N (wp / 64)
};

PoGeom po_geom(int H, int W) {
  PoGeom g;
  g.h = H - 2;
  g.w = W - 2;
  g.hp = (g.h + kPoTile - 1) / kPoTile * kPoTile;
  g.wp = (g.w + kPoTile - 1) / kPoTile * kPoTile;
  g.mt = g.hp / kPoTile;
  g.nt = g.wp / kPoTile;
  return g;
}

size_t po_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct PoLayout {
  size_t sh, sht, sw, swt, x, y, part, total;   // byte offsets into the scratch
};

PoLayout po_layout(int B, const PoGeom& g) {
  PoLayout L;
  const size_t hh = (size_t)g.hp * g.hp * sizeof(double), ww = (size_t)g.wp * g.wp * sizeof(double);
  const size_t item = (size_t)B * g.hp * g.wp * sizeof(double);
  L.sh = 0;
  L.sht = L.sh + po_align(hh);
  L.sw = L.sht + po_align(hh);
  L.swt = L.sw + po_align(ww);
  L.x = L.swt + po_align(ww);
  L.y = L.x + po_align(item);
  L.part = L.y + po_align(item);
  L.total = L.part + po_align((size_t)B * g.mt * g.nt * sizeof(double));
  return L;
}

// ---- the transform matrices ------------------------------------------------------------------------------------------------------
// S (N x N inside Np x Np, zero elsewhere) and S^T, for both axes in one launch: elements [0, hp^2) are S_h's, the rest S_w's.
__global__ __launch_bounds__(256) void poisson_dst_matrices(int h, int hp, int w, int wp, double* __restrict__ sh, double* __restrict__ sht,
                                                            double* __restrict__ sw, double* __restrict__ swt) {
  const int64_t nh = (int64_t)hp * hp, total = nh + (int64_t)wp * wp;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const bool is_h = e < nh;
    const int64_t q = is_h ? e : e - nh;
    const int Np = is_h ? hp : wp, N = is_h ? h : w;
    const int k = (int)(q / Np), n = (int)(q % Np);
    double v = 0.0;
    if (k < N && n < N) {
      const int64_t m = ((int64_t)(k + 1) * (2 * n + 1)) % (4 * (int64_t)N);   // exact: the sine's argument stays in [0, 2 pi)
      const double c = k == N - 1 ? sqrt(1.0 / (4.0 * N)) : sqrt(1.0 / (2.0 * N));
      v = c * (2.0 * sin(M_PI * (double)m / (2.0 * N)));
    }
    (is_h ? sh : sw)[(int64_t)k * Np + n] = v;
    (is_h ? sht : swt)[(int64_t)n * Np + k] = v;
  }
}

// ---- the GEMMs --------------------------------------------------------------------------------------------------------------------
struct PoArgs {
  const void* flow;       // STEP 0: gradx = component 0, grady = component 1 (element strides f_sb, f_sc, f_sr; unit columns)
  const void* bnd;        // nullable: the boundary image (b_sb, b_sr)
  void* out;              // STEP 3: [B, H, W] of the boundary's type (o_sb, o_sr)
  const double* a;        // A operand, row-major with lda; a_sb per item (0: one matrix for all)
  const double* b;        // B operand, row-major with ldb; b_sb per item
  double* c;              // C (STEPs 0 - 2), row-major with ldc; c_sb per item
  double* part;           // STEP 3: per-tile max |P|, [B][mt][nt]
  int64_t f_sb, f_sc, f_sr, b_sb, b_sr, o_sb, o_sr, a_sb, b_sb_op, c_sb;
  int lda, ldb, ldc, K;
  int H, W, h, w, hp, mt, nt;
};

// the interior divergence minus the boundary's stencil at interior pixel (i, j) of item bi, in the reference's types and order
template <typename TI, typename TO>
__device__ __forceinline__ double po_f(const PoArgs& a, int bi, int i, int j) {
  if (i >= a.h || j >= a.w) return 0.0;
  const int r = i + 1, c = j + 1;
  const TI* gx = static_cast<const TI*>(a.flow) + bi * a.f_sb;
  const TI* gy = gx + a.f_sc;
  const TI dx = gx[r * a.f_sr + c] - gx[r * a.f_sr + c - 1];
  const TI dy = gy[r * a.f_sr + c] - gy[(r - 1) * a.f_sr + c];
  double f = 0.0;   // (the reference adds both into float64 zeros)
  f = f + (double)dx;
  f = f + (double)dy;
  if (a.bnd) {
    // -4 Bd[r, c] + Bd[r, c+1] + Bd[r, c-1] + Bd[r+1, c] + Bd[r-1, c] with Bd's interior zeroed: only frame pixels count
    const TO* bd = static_cast<const TO*>(a.bnd) + bi * a.b_sb;
    const TO zero = TO(0);
    const TO right = c + 1 == a.W - 1 ? bd[r * a.b_sr + c + 1] : zero;
    const TO left = c - 1 == 0 ? bd[r * a.b_sr + c - 1] : zero;
    const TO down = r + 1 == a.H - 1 ? bd[(r + 1) * a.b_sr + c] : zero;
    const TO up = r - 1 == 0 ? bd[(r - 1) * a.b_sr + c] : zero;
    TO s = TO(-4) * zero;
    s = s + right;
    s = s + left;
    s = s + down;
    s = s + up;
    f = f - (double)s;
  }
  return f;
}

// STEP 3's frame: the boundary pixels of rows / columns this tile owns, copied (or zero) into the output; returns their max |.|
template <typename TO>
__device__ double po_frame(const PoArgs& a, int bi, int mtile, int ntile) {
  if (!(mtile == 0 || mtile == a.mt - 1 || ntile == 0 || ntile == a.nt - 1)) return 0.0;
  const int r_lo = mtile == 0 ? 0 : mtile * kPoTile + 1, r_hi = mtile == a.mt - 1 ? a.H : min(a.H, mtile * kPoTile + kPoTile + 1);
  const int c_lo = ntile == 0 ? 0 : ntile * kPoTile + 1, c_hi = ntile == a.nt - 1 ? a.W : min(a.W, ntile * kPoTile + kPoTile + 1);
  const TO* bd = a.bnd ? static_cast<const TO*>(a.bnd) + bi * a.b_sb : nullptr;
  TO* out = static_cast<TO*>(a.out) + bi * a.o_sb;
  double mx = 0.0;
  auto put = [&](int r, int c) {
    const TO v = bd ? bd[r * a.b_sr + c] : TO(0);
    out[r * a.o_sr + c] = v;
    mx = fmax(mx, fabs((double)v));
  };
  const int nr = r_hi - r_lo, nc = c_hi - c_lo;
  for (int t = threadIdx.x; t < nr; t += kPoBlock) {
    if (ntile == 0) put(r_lo + t, 0);
    if (ntile == a.nt - 1) put(r_lo + t, a.W - 1);
  }
  for (int t = threadIdx.x; t < nc; t += kPoBlock) {
    if (mtile == 0) put(0, c_lo + t);
    if (mtile == a.mt - 1) put(a.H - 1, c_lo + t);
  }
  return mx;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
  return v;
}

// STEP 0: A = F (prologue), B = S_w^T, C = T (tall: grid.y = B hp / 64).   STEP 1: A = S_h, B = T_b, C = G_b (/ D).
// STEP 2: A = S_h^T, B = G_b, C = U_b.   STEP 3: A = U (tall), B = S_w, C -> the output.   grid (N tiles, M tiles, items).
template <int STEP, typename TI, typename TO>
__global__ __launch_bounds__(kPoBlock) void poisson_gemm(PoArgs a) {
  __shared__ double s_a[2][kPoK][kPoLd];   // [k][m]
  __shared__ double s_b[2][kPoK][kPoLd];   // [k][n]
  __shared__ double s_max[kPoBlock / kWave];
  constexpr bool kTall = STEP == 0 || STEP == 3;
  const int t = threadIdx.x, lane = t % kWave, wave = t / kWave;
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lk = lane >> 4;
  const int n0 = blockIdx.x * kPoTile, m0 = blockIdx.y * kPoTile;
  const int item = kTall ? m0 / a.hp : blockIdx.z;           // (a tile never straddles two items: hp is a multiple of 64)
  const double* A = a.a + (kTall ? 0 : item * a.a_sb);
  const double* Bm = a.b + (kTall ? 0 : item * a.b_sb_op);

  // the global -> LDS assignment: A rows t / 4, k (t % 4) * 4 .. + 3;  B row t / 16, columns (t % 16) * 4 .. + 3
  const int ar = t >> 2, ak = (t & 3) * 4, bk = t >> 4, bn = (t & 15) * 4;
  double ra[4], rb[4];
  auto load = [&](int k0) {
    if constexpr (STEP == 0) {
      const int gm = m0 + ar, i = gm - item * a.hp;
#pragma unroll
      for (int j = 0; j < 4; ++j) ra[j] = po_f<TI, TO>(a, item, i, k0 + ak + j);
    } else {
      const double2* p = reinterpret_cast<const double2*>(A + (size_t)(m0 + ar) * a.lda + k0 + ak);
      const double2 q0 = p[0], q1 = p[1];
      ra[0] = q0.x;
      ra[1] = q0.y;
      ra[2] = q1.x;
      ra[3] = q1.y;
    }
    const double2* p = reinterpret_cast<const double2*>(Bm + (size_t)(k0 + bk) * a.ldb + n0 + bn);
    const double2 q0 = p[0], q1 = p[1];
    rb[0] = q0.x;
    rb[1] = q0.y;
    rb[2] = q1.x;
    rb[3] = q1.y;
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s_a[buf][ak + j][ar] = ra[j];
    *reinterpret_cast<double2*>(&s_b[buf][bk][bn]) = make_double2(rb[0], rb[1]);
    *reinterpret_cast<double2*>(&s_b[buf][bk][bn + 2]) = make_double2(rb[2], rb[3]);
  };

  po_acc acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = po_acc{0.0, 0.0, 0.0, 0.0};

  const int steps = a.K / kPoK;
  load(0);
  store(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    if (s + 1 < steps) load((s + 1) * kPoK);   // in flight during this step's MFMAs
#pragma unroll
    for (int kk = 0; kk < kPoK / 4; ++kk) {
      const int k = kk * 4 + lk;
      const double a0 = s_a[buf][k][wm * 32 + lr], a1 = s_a[buf][k][wm * 32 + 16 + lr];
      const double b0 = s_b[buf][k][wn * 32 + lr], b1 = s_b[buf][k][wn * 32 + 16 + lr];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (s + 1 < steps) store(buf ^ 1);   // (buf ^ 1 was last read in step s - 1, before the previous barrier)
    __syncthreads();
  }

  // epilogue: element r of acc[i][j] is row m0 + wm 32 + i 16 + lk + 4 r, column n0 + wn 32 + j 16 + lr
  if constexpr (STEP == 3) {
    const int mtile = (m0 - item * a.hp) / kPoTile, ntile = blockIdx.x;
    TO* out = static_cast<TO*>(a.out) + item * a.o_sb;
    double mx = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 - item * a.hp + wm * 32 + i * 16 + lk + 4 * r, col = n0 + wn * 32 + j * 16 + lr;
          if (row < a.h && col < a.w) {
            const TO v = (TO)acc[i][j][r];
            out[(row + 1) * a.o_sr + col + 1] = v;
            mx = fmax(mx, fabs((double)v));
          }
        }
    mx = fmax(mx, po_frame<TO>(a, item, mtile, ntile));
    mx = wave_max(mx);
    if (lane == 0) s_max[wave] = mx;
    __syncthreads();
    if (t == 0) {
      double m = s_max[0];
      for (int k = 1; k < kPoBlock / kWave; ++k) m = fmax(m, s_max[k]);
      a.part[((size_t)item * a.mt + mtile) * a.nt + ntile] = m;
    }
  } else {
    double* C = a.c + (kTall ? 0 : item * a.c_sb);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + wm * 32 + i * 16 + lk + 4 * r, col = n0 + wn * 32 + j * 16 + lr;
          double v = acc[i][j][r];
          if constexpr (STEP == 1) {
            if (row < a.h && col < a.w) {
              const double d = (2.0 * cos(M_PI * (double)(col + 1) / (double)a.W) - 2.0) +
                               (2.0 * cos(M_PI * (double)(row + 1) / (double)a.H) - 2.0);
              v = v / d;
            } else {
              v = 0.0;   // (the padding stays zero for the next two products)
            }
          }
          C[(size_t)row * a.ldc + col] = v;
        }
  }
}

// ---- the uint8 picture ------------------------------------------------------------------------------------------------------------
// (P - 0) / max|P| * (255 - 128) + 128 in the output type, truncated (src/utils/frame_utils.py:39-53 then .astype(np.uint8));
// an all-zero P gives 128 everywhere (the reference divides 0 by 0 and casts NaN).  grid (pixel chunks, items).
template <typename TO>
__global__ __launch_bounds__(kPoImgBlock) void poisson_image(const TO* __restrict__ p, int64_t o_sb, int64_t o_sr, int H, int W,
                                                             const double* __restrict__ part, int tiles, uint8_t* __restrict__ img) {
  __shared__ double s_max[kPoImgBlock / kWave];
  const int b = blockIdx.y, t = threadIdx.x;
  double m = 0.0;
  for (int k = t; k < tiles; k += kPoImgBlock) m = fmax(m, part[(size_t)b * tiles + k]);
  m = wave_max(m);
  if (t % kWave == 0) s_max[t / kWave] = m;
  __syncthreads();
  for (int k = 0; k < kPoImgBlock / kWave; ++k) m = fmax(m, s_max[k]);
  const TO mx = (TO)m;   // (exact: the partials are |values| of the output type)
  const int64_t n = (int64_t)H * W;
  const int64_t base = (int64_t)blockIdx.x * kPoImgBlock * kPoImgPix;
#pragma unroll
  for (int q = 0; q < kPoImgPix; ++q) {
    const int64_t e = base + q * kPoImgBlock + t;
    if (e >= n) break;
    const int r = (int)(e / W), c = (int)(e % W);
    uint8_t u = 128;
    if (mx != TO(0)) {
      const TO v = p[b * o_sb + r * o_sr + c];
      const TO s = ((v - TO(0)) / mx) * TO(127) + TO(128);
      u = s >= TO(0) ? (uint8_t)(int)s : (uint8_t)0;   // (s is in [1, 255]; NaN -> 0)
    }
    img[(size_t)b * n + e] = u;
  }
}

template <typename TI, typename TO>
int po_launch(PoArgs a, int B, const PoGeom& g, const PoLayout& L, char* scratch, uint8_t* img, hipStream_t s) {
  double* sh = reinterpret_cast<double*>(scratch + L.sh);
  double* sht = reinterpret_cast<double*>(scratch + L.sht);
  double* sw = reinterpret_cast<double*>(scratch + L.sw);
  double* swt = reinterpret_cast<double*>(scratch + L.swt);
  double* x = reinterpret_cast<double*>(scratch + L.x);
  double* y = reinterpret_cast<double*>(scratch + L.y);
  a.part = reinterpret_cast<double*>(scratch + L.part);
  const int64_t elems = (int64_t)g.hp * g.hp + (int64_t)g.wp * g.wp;
  hipLaunchKernelGGL(poisson_dst_matrices, dim3(stream_grid(elems, 256)), dim3(256), 0, s, g.h, g.hp, g.w, g.wp, sh, sht, sw, swt);
  EBOS_CHECK_LAUNCH("ebos_poisson_reconstruct: poisson_dst_matrices");
  const int64_t item = (int64_t)g.hp * g.wp;
  const dim3 tall(g.nt, B * g.mt, 1), batched(g.nt, g.mt, B), block(kPoBlock);

  a.a = nullptr;   // T = F S_w^T
  a.a_sb = 0;
  a.b = swt;
  a.b_sb_op = 0;
  a.ldb = g.wp;
  a.c = x;
  a.ldc = g.wp;
  a.c_sb = 0;
  a.K = g.wp;
  hipLaunchKernelGGL((poisson_gemm<0, TI, TO>), tall, block, 0, s, a);
  EBOS_CHECK_LAUNCH("ebos_poisson_reconstruct: poisson_gemm<0>");

  a.a = sh;   // G = (S_h T) / D
  a.lda = g.hp;
  a.b = x;
  a.b_sb_op = item;
  a.c = y;
  a.c_sb = item;
  a.K = g.hp;
  hipLaunchKernelGGL((poisson_gemm<1, TI, TO>), batched, block, 0, s, a);
  EBOS_CHECK_LAUNCH("ebos_poisson_reconstruct: poisson_gemm<1>");

  a.a = sht;   // U = S_h^T G
  a.b = y;
  a.c = x;
  hipLaunchKernelGGL((poisson_gemm<2, TI, TO>), batched, block, 0, s, a);
  EBOS_CHECK_LAUNCH("ebos_poisson_reconstruct: poisson_gemm<2>");

  a.a = x;   // P = U S_w
  a.lda = g.wp;
  a.b = sw;
  a.b_sb_op = 0;
  a.c = nullptr;
  a.c_sb = 0;
  a.K = g.wp;
  hipLaunchKernelGGL((poisson_gemm<3, TI, TO>), tall, block, 0, s, a);
  EBOS_CHECK_LAUNCH("ebos_poisson_reconstruct: poisson_gemm<3>");

  if (img) {
    const int64_t n = (int64_t)a.H * a.W;
    const dim3 grid((unsigned)((n + kPoImgBlock * kPoImgPix - 1) / (kPoImgBlock * kPoImgPix)), B);
    hipLaunchKernelGGL((poisson_image<TO>), grid, dim3(kPoImgBlock), 0, s, static_cast<const TO*>(a.out), a.o_sb, a.o_sr, a.H, a.W,
                       a.part, g.mt * g.nt, img);
    EBOS_CHECK_LAUNCH("ebos_poisson_reconstruct: poisson_image");
  }
  return EBOS_OK;
}

}  // namespace
}  // namespace ebos

extern "C" {

size_t ebos_poisson_scratch_bytes(int B, int H, int W) {
  if (B <= 0 || H < 3 || W < 3) return 0;
  const ebos::PoGeom g = ebos::po_geom(H, W);
  return ebos::po_layout(B, g).total;
}

int ebos_poisson_reconstruct(int in_dtype, int out_dtype, int B, int H, int W, const void* flow, int64_t flow_sb, int64_t flow_sc,
                             int64_t flow_sr, const void* boundary, int64_t bnd_sb, int64_t bnd_sr, void* out, int64_t out_sb,
                             int64_t out_sr, uint8_t* out_u8, void* scratch, size_t scratch_bytes, ebos_stream_t stream) {
  using namespace ebos;
  EBOS_REQUIRE((in_dtype == EBOS_POISSON_F32 || in_dtype == EBOS_POISSON_F64) && (out_dtype == EBOS_POISSON_F32 || out_dtype == EBOS_POISSON_F64),
               "ebos_poisson_reconstruct: dtypes %d / %d are not F32 (0) or F64 (1)", in_dtype, out_dtype);
  EBOS_REQUIRE(B > 0 && H >= 3 && W >= 3 && (int64_t)H * W < ((int64_t)1 << 31), "ebos_poisson_reconstruct: bad shape B = %d, H = %d, W = %d",
               B, H, W);
  const PoGeom g = po_geom(H, W);
  EBOS_REQUIRE(B <= 65535 && (int64_t)B * g.mt <= 65535 && (int64_t)B * g.hp * g.wp < ((int64_t)1 << 40),
               "ebos_poisson_reconstruct: batch of %d at %d x %d is too large for one call", B, H, W);
  EBOS_REQUIRE(flow && out && scratch, "ebos_poisson_reconstruct: NULL buffer");
  EBOS_REQUIRE(flow_sb >= 0 && flow_sc >= 0 && flow_sr >= W && bnd_sb >= 0 && out_sb >= 0 && out_sr >= W && (!boundary || bnd_sr >= W),
               "ebos_poisson_reconstruct: bad strides");
  const size_t need = ebos_poisson_scratch_bytes(B, H, W);
  if (scratch_bytes < need) {
    set_error("ebos_poisson_reconstruct: scratch too small (%zu < %zu)", scratch_bytes, need);
    return EBOS_ERR_SCRATCH;
  }
  EBOS_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 16 == 0, "ebos_poisson_reconstruct: scratch not 16-byte aligned");
  PoArgs a = {};
  a.flow = flow;
  a.bnd = boundary;
  a.out = out;
  a.f_sb = flow_sb;
  a.f_sc = flow_sc;
  a.f_sr = flow_sr;
  a.b_sb = bnd_sb;
  a.b_sr = bnd_sr;
  a.o_sb = out_sb;
  a.o_sr = out_sr;
  a.H = H;
  a.W = W;
  a.h = g.h;
  a.w = g.w;
  a.hp = g.hp;
  a.mt = g.mt;
  a.nt = g.nt;
  const PoLayout L = po_layout(B, g);
  char* s = static_cast<char*>(scratch);
  const hipStream_t st = as_stream(stream);
  if (in_dtype == EBOS_POISSON_F64)
    return out_dtype == EBOS_POISSON_F64 ? po_launch<double, double>(a, B, g, L, s, out_u8, st) : po_launch<double, float>(a, B, g, L, s, out_u8, st);
  return out_dtype == EBOS_POISSON_F64 ? po_launch<float, double>(a, B, g, L, s, out_u8, st) : po_launch<float, float>(a, B, g, L, s, out_u8, st);
}

}  // extern "C"

// Conjugate gradients on the normal equations (CGLS) of Wald's consistency A(f) = LR MS, per plane: the pieces that
// fir_decimate (A p) and fir_decimate_adjoint (A^T r - damp d) of mtf.hip leave open -- per-plane dot products and vector
// updates whose coefficients never leave the device.  Host definition: tmdiff_amd/metrics.py, consistency_solve; the driver
// that strings the launches together: tmdiff_amd/ops.py, consistency_solve.  Dense fp32 planes [planes, n], n the element
// count of a plane; nothing is allocated or read back, no atomics, no fences: a call can be captured into a graph.
//
// CHUNKS.  A plane of n elements is cut into `count` chunks of `chunk` elements, and both depend on n alone:
//   want = min(ceil(n / 4096), 256),  chunk = ceil(n / want) rounded up to a multiple of 1024,  count = max(1, ceil(n / chunk))
// (1024 x 1024: 256 chunks of 4096; 64 x 64: one chunk; never more than 256, one per lane of the workgroup that adds them up).
// One 256-lane workgroup walks one chunk of one plane; blockIdx.y strides the planes.  Lane t takes the elements
// e0 + 1024 k + 4 t + {0, 1, 2, 3}, k = 0, 1, ...: a 16-byte access when n % 4 == 0 and the pointers are 16-byte aligned, four
// dwords otherwise -- the same elements in the same lanes either way.
//
// SUMMATION ORDER of <a, b> over a plane, the same wherever it is made (tmdiff_plane_dots, the ||r||^2 inside tmdiff_cg_step, the
// <p, p> inside tmdiff_cg_direction): a lane starts at acc = 0.0 and adds its products in ascending element index,
// acc = fma((double)a, (double)b, acc) -- the product of two floats is exact in double, so a step is one rounding; the lanes of
// a chunk are added by the workgroup sum of stats.h (xor butterfly inside a wave, then the waves in ascending order); that is the
// chunk's PARTIAL SUM, partials[plane * count + chunk].  The plane's total is the workgroup sum of stats.h over the partials,
// partial c in lane c and 0.0 in the lanes from `count` on.  It depends on n alone: not on the grid, the batch, the alignment or
// on which kernel adds.  There is no finalize launch between a dot and its consumer: every workgroup of the consumer adds the
// partials of its plane itself, and all of them get identical bits.  tmdiff_plane_totals writes totals for a caller who wants
// them in memory (ops.plane_dots, the ||r||^2 trace at the end of a solve).
//
// COEFFICIENTS.  alpha = gamma / (qq + damp * pp) and beta = gamma_new / gamma_old are formed in double from those totals (the
// product damp * pp and the sum rounded separately), are EXACTLY 0 when the denominator is 0 (a plane that is already consistent
// has r = s = p = q = 0: it keeps d = 0 and produces no NaN, whatever the other planes of the batch do), and are rounded to
// float once.  Every element then takes one fused multiply-add:
//   tmdiff_cg_step:       d = fma(alpha, p, d)  (first step: d = alpha * p, d is not read),  r = fma(-alpha, q, r)
//   tmdiff_cg_direction:  p = fma(beta, p, s)
#include <algorithm>

#include "stats.h"

namespace {

constexpr int NT = 256;            // lanes of a workgroup
constexpr int MAXP = NT;           // most partial sums of a plane: one per lane of the workgroup that adds them
constexpr int GRID_TARGET = 4096;  // workgroups of a launch before blockIdx.y starts to stride the planes

struct Chunks {
  int chunk, count;
};
inline Chunks plane_chunks(int n) {
  const long want = std::max<long>(std::min<long>(((long)n + 4095) / 4096, MAXP), 1);
  const long chunk = std::max<long>(((n + want - 1) / want + 1023) / 1024 * 1024, 1024);
  return {(int)chunk, (int)std::max<long>((n + chunk - 1) / chunk, 1)};
}

inline bool vec_ok(int n, std::initializer_list<const void*> ptrs) {
  bool ok = n % 4 == 0;
  for (const void* p : ptrs) ok = ok && tmdiff::aligned16(p);
  return ok;
}

inline unsigned planes_y(int planes, int blocks_x) { return (unsigned)std::max(1, std::min(planes, GRID_TARGET / blocks_x)); }

// The four elements at i .. i + 3 of a plane of n (i a multiple of 4, i < n); elements from n on read as 0 and are not stored.
__device__ __forceinline__ float4 load4(const float* p, long i, int n, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(p + i);
  float4 v;
  v.x = p[i];
  v.y = i + 1 < n ? p[i + 1] : 0.f;
  v.z = i + 2 < n ? p[i + 2] : 0.f;
  v.w = i + 3 < n ? p[i + 3] : 0.f;
  return v;
}
__device__ __forceinline__ void store4(float* p, long i, int n, bool vec, float4 v) {
  if (vec) {
    *reinterpret_cast<float4*>(p + i) = v;
    return;
  }
  p[i] = v.x;
  if (i + 1 < n) p[i + 1] = v.y;
  if (i + 2 < n) p[i + 2] = v.z;
  if (i + 3 < n) p[i + 3] = v.w;
}
// A lane's step of the summation order: elements past the plane's end arrive as zeros and change no bit (acc starts at +0).
__device__ __forceinline__ double dot4(float4 a, float4 b, double acc) {
  acc = fma((double)a.x, (double)b.x, acc);
  acc = fma((double)a.y, (double)b.y, acc);
  acc = fma((double)a.z, (double)b.z, acc);
  return fma((double)a.w, (double)b.w, acc);
}

// The totals of K dots of plane pl from their partial sums (count[k] of them for dot k; a null list totals 0), in every lane: one
// barrier for all K.  The caller syncs before `red` (K doubles per wave) is reused.
template <int K>
__device__ __forceinline__ void plane_totals(const double* const (&partials)[K], const int (&count)[K], int pl, double (&tot)[K],
                                             double* red) {
#pragma unroll
  for (int k = 0; k < K; ++k)
    tot[k] = partials[k] && (int)threadIdx.x < count[k] ? partials[k][(long)pl * count[k] + threadIdx.x] : 0.0;
  tmdiff::wg_sum<NT / 64, K, K>(tot, red);
}

// partials of <a0, b0> (blockIdx.x < count0, planes of n0) and of <a1, b1> (the blocks after them, planes of n1)
struct DotArgs {
  const float *a0, *b0, *a1, *b1;
  double *out0, *out1;
  int n0, n1, chunk0, chunk1, count0, count1, vec0, vec1, planes;
};

__global__ void __launch_bounds__(NT) plane_dots_kernel(DotArgs A) {
  __shared__ double red[NT / 64];
  const bool second = (int)blockIdx.x >= A.count0;
  const float* a = second ? A.a1 : A.a0;
  const float* b = second ? A.b1 : A.b0;
  double* out = second ? A.out1 : A.out0;
  const int n = second ? A.n1 : A.n0, chunk = second ? A.chunk1 : A.chunk0, count = second ? A.count1 : A.count0;
  const bool vec = second ? A.vec1 : A.vec0;
  const int c = second ? blockIdx.x - A.count0 : blockIdx.x;
  const long e0 = (long)c * chunk, e1 = min(e0 + chunk, (long)n);
  for (int pl = blockIdx.y; pl < A.planes; pl += gridDim.y) {
    const float* ap = a + (long)pl * n;
    const float* bp = b + (long)pl * n;
    double acc = 0.0;
    for (long i = e0 + 4 * threadIdx.x; i < e1; i += 4 * NT) {
      const float4 va = load4(ap, i, n, vec);
      acc = dot4(va, a == b ? va : load4(bp, i, n, vec), acc);
    }
    acc = tmdiff::block_sum_f64(acc, red);
    if (threadIdx.x == 0) out[(long)pl * count + c] = acc;
    __syncthreads();   // the next plane overwrites red
  }
}

// out[pl * items + k] = the total of partials[k * item_stride + pl * count ..], k < items
__global__ void __launch_bounds__(NT) plane_totals_kernel(const double* __restrict__ partials, double* __restrict__ out, int planes,
                                                          int count, int items, long item_stride) {
  __shared__ double red[NT / 64];
  for (int pl = blockIdx.x; pl < planes; pl += gridDim.x)
    for (int k = 0; k < items; ++k) {
      const double* const src[1] = {partials + k * item_stride};
      const int counts[1] = {count};
      double tot[1];
      plane_totals<1>(src, counts, pl, tot, red);
      if (threadIdx.x == 0) out[(long)pl * items + k] = tot[0];
      __syncthreads();
    }
}

struct StepArgs {
  const float *p, *q;
  float *d, *r;
  const double *gamma, *qq, *pp;   // partial sums: <s, s> and <p, p> over the full extent, <q, q> over the low one
  double* rr;                      // partial sums of the new <r, r>
  double damp;
  int nf, nl, chunk_f, chunk_l, count_f, count_l, vec_f, vec_l, planes, first;
};

// blockIdx.x < count_f: d of a chunk of the full extent; the blocks after them: r of a chunk of the low extent and its <r, r>
__global__ void __launch_bounds__(NT) cg_step_kernel(StepArgs A) {
  __shared__ double red[3 * (NT / 64)];
  __shared__ double red_r[NT / 64];
  const bool low = (int)blockIdx.x >= A.count_f;
  const int c = low ? blockIdx.x - A.count_f : blockIdx.x;
  const int n = low ? A.nl : A.nf, chunk = low ? A.chunk_l : A.chunk_f;
  const bool vec = low ? A.vec_l : A.vec_f;
  const long e0 = (long)c * chunk, e1 = min(e0 + chunk, (long)n);
  for (int pl = blockIdx.y; pl < A.planes; pl += gridDim.y) {
    double tot[3];   // gamma, <q, q>, <p, p>
    const double* const src[3] = {A.gamma, A.qq, A.damp != 0.0 ? A.pp : nullptr};
    const int counts[3] = {A.count_f, A.count_l, A.count_f};
    plane_totals<3>(src, counts, pl, tot, red);
    const double delta = A.damp != 0.0 ? __dadd_rn(tot[1], __dmul_rn(A.damp, tot[2])) : tot[1];
    const float alpha = delta == 0.0 ? 0.f : (float)(tot[0] / delta);
    if (!low) {
      const float* pp = A.p + (long)pl * n;
      float* dp = A.d + (long)pl * n;
      for (long i = e0 + 4 * threadIdx.x; i < e1; i += 4 * NT) {
        const float4 vp = load4(pp, i, n, vec);
        float4 vd;
        if (A.first) {
          vd = make_float4(__fmul_rn(alpha, vp.x), __fmul_rn(alpha, vp.y), __fmul_rn(alpha, vp.z), __fmul_rn(alpha, vp.w));
        } else {
          vd = load4(dp, i, n, vec);
          vd = make_float4(__fmaf_rn(alpha, vp.x, vd.x), __fmaf_rn(alpha, vp.y, vd.y), __fmaf_rn(alpha, vp.z, vd.z),
                           __fmaf_rn(alpha, vp.w, vd.w));
        }
        store4(dp, i, n, vec, vd);
      }
    } else {
      const float* qp = A.q + (long)pl * n;
      float* rp = A.r + (long)pl * n;
      double acc = 0.0;
      for (long i = e0 + 4 * threadIdx.x; i < e1; i += 4 * NT) {
        const float4 vq = load4(qp, i, n, vec);
        float4 vr = load4(rp, i, n, vec);
        vr = make_float4(__fmaf_rn(-alpha, vq.x, vr.x), __fmaf_rn(-alpha, vq.y, vr.y), __fmaf_rn(-alpha, vq.z, vr.z),
                         __fmaf_rn(-alpha, vq.w, vr.w));
        store4(rp, i, n, vec, vr);
        acc = dot4(vr, vr, acc);
      }
      acc = tmdiff::block_sum_f64(acc, red_r);
      if (threadIdx.x == 0) A.rr[(long)pl * A.count_l + c] = acc;
    }
    __syncthreads();   // the next plane overwrites red and red_r
  }
}

struct DirArgs {
  const float* s;
  float* p;
  const double *gamma_new, *gamma_old;   // partial sums of <s, s>: this step's and the one before
  double* pp;                            // partial sums of the new <p, p>, or null (damp == 0: nobody reads them)
  int n, chunk, count, vec, planes;
};

__global__ void __launch_bounds__(NT) cg_direction_kernel(DirArgs A) {
  __shared__ double red[2 * (NT / 64)];
  __shared__ double red_p[NT / 64];
  const int c = blockIdx.x, n = A.n;
  const bool vec = A.vec;
  const long e0 = (long)c * A.chunk, e1 = min(e0 + A.chunk, (long)n);
  for (int pl = blockIdx.y; pl < A.planes; pl += gridDim.y) {
    double tg[2];
    const double* const src[2] = {A.gamma_new, A.gamma_old};
    const int counts[2] = {A.count, A.count};
    plane_totals<2>(src, counts, pl, tg, red);
    const float beta = tg[1] == 0.0 ? 0.f : (float)(tg[0] / tg[1]);
    const float* sp = A.s + (long)pl * n;
    float* pp = A.p + (long)pl * n;
    double acc = 0.0;
    for (long i = e0 + 4 * threadIdx.x; i < e1; i += 4 * NT) {
      const float4 vs = load4(sp, i, n, vec);
      float4 vp = load4(pp, i, n, vec);
      vp = make_float4(__fmaf_rn(beta, vp.x, vs.x), __fmaf_rn(beta, vp.y, vs.y), __fmaf_rn(beta, vp.z, vs.z), __fmaf_rn(beta, vp.w, vs.w));
      store4(pp, i, n, vec, vp);
      if (A.pp) acc = dot4(vp, vp, acc);   // uniform: without damp nobody reads <p, p>
    }
    if (A.pp) {
      acc = tmdiff::block_sum_f64(acc, red_p);
      if (threadIdx.x == 0) A.pp[(long)pl * A.count + c] = acc;
    }
    __syncthreads();   // the next plane overwrites red and red_p
  }
}

const char* kLimits = "planes >= 0, 0 <= n <= 2^31 - 1 elements per plane and planes * n <= 2^31 - 1";

int plane_limits(const char* name, int planes, int n) {
  if (planes < 0 || n < 0 || !tmdiff::fits_int32((double)planes * n))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "%s: planes=%d n=%d (%s)", name, planes, n, kLimits);
  return TMDIFF_OK;
}

}  // namespace

extern "C" {

int32_t tmdiff_plane_dots_partials(int32_t n) { return n < 0 ? 0 : plane_chunks(n).count; }

int tmdiff_plane_dots(const float* a0, const float* b0, int32_t n0, double* partials0, const float* a1, const float* b1, int32_t n1,
                      double* partials1, int32_t planes, tmdiff_stream_t stream) {
  if (const int rc = plane_limits("plane_dots", planes, n0)) return rc;
  const bool two = partials1 != nullptr;
  if (two)
    if (const int rc = plane_limits("plane_dots", planes, n1)) return rc;
  if (planes == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(partials0 && ((a0 && b0) || n0 == 0) && (!two || (a1 && b1) || n1 == 0), "plane_dots: null tensor");
  TMDIFF_REQUIRE(((reinterpret_cast<uintptr_t>(partials0) | reinterpret_cast<uintptr_t>(partials1)) & 7u) == 0,
                 "plane_dots: partial sums must be 8-byte aligned");
  const Chunks c0 = plane_chunks(n0), c1 = two ? plane_chunks(n1) : Chunks{1024, 0};
  DotArgs A{a0, b0, a1, b1, partials0, partials1, n0, two ? n1 : 0, c0.chunk, c1.chunk, c0.count, c1.count, vec_ok(n0, {a0, b0}),
            two && vec_ok(n1, {a1, b1}), planes};
  const int bx = c0.count + c1.count;
  plane_dots_kernel<<<dim3((unsigned)bx, planes_y(planes, bx)), NT, 0, tmdiff::as_stream(stream)>>>(A);
  return tmdiff::check_launch("plane_dots");
}

int tmdiff_plane_totals(const double* partials, double* out, int32_t planes, int32_t count, int32_t items, int64_t item_stride,
                        tmdiff_stream_t stream) {
  if (planes < 0 || count < 1 || count > MAXP || items < 0 || item_stride < 0)
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "plane_totals: planes=%d count=%d items=%d item_stride=%lld (planes, items, item_stride >= 0, "
                        "1 <= count <= %d)", planes, count, items, (long long)item_stride, MAXP);
  if (planes == 0 || items == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(partials && out, "plane_totals: null tensor");
  plane_totals_kernel<<<(unsigned)std::min(planes, GRID_TARGET), NT, 0, tmdiff::as_stream(stream)>>>(partials, out, planes, count, items,
                                                                                                   item_stride);
  return tmdiff::check_launch("plane_totals");
}

int tmdiff_cg_step(const float* p, const float* q, float* d, float* r, const double* gamma, const double* qq, const double* pp,
                   double damp, double* rr, int32_t planes, int32_t n_full, int32_t n_low, int32_t first, tmdiff_stream_t stream) {
  if (const int rc = plane_limits("cg_step", planes, n_full)) return rc;
  if (const int rc = plane_limits("cg_step", planes, n_low)) return rc;
  if (!(damp >= 0.0)) return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "cg_step: damp=%g (damp >= 0)", damp);
  if (planes == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(gamma && qq && rr && (pp || damp == 0.0) && ((p && d) || n_full == 0) && ((q && r) || n_low == 0), "cg_step: null tensor");
  const Chunks cf = plane_chunks(n_full), cl = plane_chunks(n_low);
  StepArgs A{p, q, d, r, gamma, qq, pp, rr, damp, n_full, n_low, cf.chunk, cl.chunk, cf.count, cl.count, vec_ok(n_full, {p, d}),
             vec_ok(n_low, {q, r}), planes, first != 0};
  const int bx = cf.count + cl.count;
  cg_step_kernel<<<dim3((unsigned)bx, planes_y(planes, bx)), NT, 0, tmdiff::as_stream(stream)>>>(A);
  return tmdiff::check_launch("cg_step");
}

int tmdiff_cg_direction(const float* s, float* p, const double* gamma_new, const double* gamma_old, double* pp, int32_t planes,
                        int32_t n_full, tmdiff_stream_t stream) {
  if (const int rc = plane_limits("cg_direction", planes, n_full)) return rc;
  if (planes == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(gamma_new && gamma_old && ((s && p) || n_full == 0), "cg_direction: null tensor");
  const Chunks cf = plane_chunks(n_full);
  DirArgs A{s, p, gamma_new, gamma_old, pp, n_full, cf.chunk, cf.count, vec_ok(n_full, {s, p}), planes};
  cg_direction_kernel<<<dim3((unsigned)cf.count, planes_y(planes, cf.count)), NT, 0, tmdiff::as_stream(stream)>>>(A);
  return tmdiff::check_launch("cg_direction");
}

}  // extern "C"

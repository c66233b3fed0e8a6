// Sampler-side elementwise kernels for gfx950 (all HBM-bound, 16 B per lane):
//   DDPM reverse step, DPM-Solver linear combinations, x0 prediction, dynamic thresholding
//   (per-sample |x| quantile by radix select), q_sample, add.
// Reference: GeneralModel/diffusion_general.py:134-138, :192-208, :341-347, :376-378;
//            core/dpm_solver_pytorch.py:302-306, :430-456, :563-927; utils/util.py:135-142.
// Arithmetic is in the reference's evaluation order with every product rounded on its own (mul_rounded below: no FMA
// contraction), so a step differs from the PyTorch CPU path only through eps itself.  The one exception is axpby, whose
// accumulation is an explicit fma per term (see axpby_kernel).
// Two loops carry every kernel but q_sample and the quantile select:
//   FOR_EACH_VEC / launch_elementwise: the grid-stride pass of the single-tensor kernels (DDPM step, axpby, x0, add), V = 4
//     floats per lane where every operand is 16-byte aligned and n % 4 == 0, else V = 1; a kernel is its arithmetic on
//     float[V] operands between load<V> and store<V>.
//   chunk_of / walk_chunk: the multi-tensor kernels (EMA axpby, AdamW, squared norm): one workgroup per chunk of one tensor,
//     16 bytes per lane and a scalar tail where the tensor's pointers are aligned, scalar throughout where not.
#include <initializer_list>

#include "stats.h"

namespace {
using tmdiff::aligned16;

// V consecutive floats at p: one 16-byte access for V = 4 (p 16-byte aligned), one dword for V = 1
template <int V>
__device__ __forceinline__ void load(float (&v)[V], const float* p) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(p);
  else v[0] = *p;
}
template <int V>
__device__ __forceinline__ void store(float* p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = *reinterpret_cast<const float4*>(v);
  else *p = v[0];
}
using Vec4 = std::integral_constant<int, 4>;
using Vec1 = std::integral_constant<int, 1>;

// THE grid-stride loop of the single-tensor kernels over vectors i < nvec (workgroups of 256, grid_for below).  A macro on
// purpose, as TMDIFF_SEGMENT_OF (common.h): with the body handed to a function (a lambda by reference or by value, a functor)
// x0_kernel<4> compiled to other instructions (packed products and sums in place of scalar ones); as text, every kernel keeps
// the instructions it had with the loop written out.
#define FOR_EACH_VEC(i, nvec) for (long i = blockIdx.x * 256L + threadIdx.x; i < (nvec); i += 256L * gridDim.x)

inline int grid_for(long nvec) {
  long blocks = (nvec + 255) / 256;
  return (int)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));
}

inline bool all_aligned(std::initializer_list<const void*> ps, long n) {
  if (n % 4) return false;
  for (const void* p : ps)
    if (p && !aligned16(p)) return false;
  return true;
}

// ... and THE launch: launch(Vec4 / Vec1, grid, nvec) starts the kernel's 16-byte instantiation where n % 4 == 0 and every
// operand that is not NULL is 16-byte aligned, else the scalar one.
template <class L>
int launch_elementwise(std::initializer_list<const void*> operands, long n, const char* name, L&& launch) {
  if (all_aligned(operands, n)) launch(Vec4{}, grid_for(n / 4), n / 4);
  else launch(Vec1{}, grid_for(n), n);
  return tmdiff::check_launch(name);
}

// a * b rounded to fp32 on its own.  __fmul_rn is a plain product to the compiler, which contracts it into the add or subtract
// that consumes it (v_fma_f32 / v_pk_fma_f32) -- and not alike in the 16-byte and the scalar loop of one kernel.  A product
// formed under this pragma stays a product.  Every product of the elementwise kernels (axpby's fma apart) and of the AdamW
// update below goes through here: each expression is mul, mul, add as PyTorch evaluates the reference's, an aligned and an
// unaligned tensor get the same bits, and the gradient-scaled AdamW step is the plain step on g * coef bit for bit.
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

struct DdpmCoef {
  float c_recip, c_recipm1, coef1, coef2, sigma;
  int clip;
};

__device__ __forceinline__ float ddpm_one(float x, float e, float nz, const DdpmCoef& k) {
  float x0 = __fsub_rn(mul_rounded(k.c_recip, x), mul_rounded(k.c_recipm1, e));     // predict_start_from_noise
  if (k.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);                                     // clamp_(-1, 1)
  const float mean = __fadd_rn(mul_rounded(k.coef1, x0), mul_rounded(k.coef2, x));  // q_posterior
  return __fadd_rn(mean, mul_rounded(nz, k.sigma));                                 // + noise * exp(0.5 logvar)
}

// One grid-stride pass of the DDPM update (shared by the host-scalar and the device-scalar kernels, so both round
// identically).  No __restrict__ on x / out: the device-scalar kernel updates x in place (element i is read before it
// is written, by the same lane).
template <int V>
__device__ __forceinline__ void ddpm_step_body(const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                               const float* __restrict__ ms, float* out, float* __restrict__ img, long nvec,
                                               const DdpmCoef& k) {
  FOR_EACH_VEC(i, nvec) {
    float xv[V], ev[V], nv[V], mv[V], ov[V];
    load<V>(xv, x + i * V);
    load<V>(ev, eps + i * V);
    if (noise) load<V>(nv, noise + i * V);
    if (img) load<V>(mv, ms + i * V);
#pragma unroll
    for (int j = 0; j < V; ++j) ov[j] = ddpm_one(xv[j], ev[j], noise ? nv[j] : 0.f, k);
    store<V>(out + i * V, ov);
    if (!img) continue;
#pragma unroll
    for (int j = 0; j < V; ++j) mv[j] = ov[j] + mv[j];
    store<V>(img + i * V, mv);
  }
}

template <int V>
__global__ void __launch_bounds__(256) ddpm_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                        const float* __restrict__ noise, const float* __restrict__ ms,
                                                        float* __restrict__ out, float* __restrict__ img, long nvec,
                                                        DdpmCoef k) {
  ddpm_step_body<V>(x, eps, noise, ms, out, img, nvec, k);
}

// Slot of p_sample_loop's frame stack that step t fills: slot 0 is the initial x_T + MS, then one slot per kept step
// (t % every == 0) in the order the loop visits them (t = T-1 down to 0).
__host__ __device__ __forceinline__ int ddpm_frame_slot(int t, int T, int every) { return 1 + (T - 1) / every - t / every; }

// The same step with its scalars read from device memory: t = *step (one word every lane reads: a uniform load), then
// row t of the coefficient table.  Every branch below depends on t only, so it is the same for the whole grid.
template <int V>
__global__ void __launch_bounds__(256) ddpm_step_dev_kernel(const float* x, const float* __restrict__ eps,
                                                            const float* __restrict__ noise, const float* __restrict__ ms,
                                                            float* out, float* __restrict__ frames, long nvec, long n,
                                                            const int32_t* __restrict__ step, const float* __restrict__ coef,
                                                            int T, int frame_every, int clip) {
  const int t = *step;
  if (t < 0 || t >= T) return;
  const float* c = coef + 5L * t;
  const DdpmCoef k{c[0], c[1], c[2], c[3], c[4], clip};
  float* img = frames && t % frame_every == 0 ? frames + (long)ddpm_frame_slot(t, T, frame_every) * n : nullptr;
  ddpm_step_body<V>(x, eps, k.sigma != 0.f ? noise : nullptr, ms, out, img, nvec, k);
}

// Advance the sampler's step word and write the [B, 1] time input the next network evaluation reads (t + 1, exact in
// fp32).  One workgroup; launched after the step kernel in stream order.
__global__ void __launch_bounds__(256) sampler_tick_kernel(int32_t* step, float* time_in, int B, int set_to) {
  __shared__ int t_new;
  if (threadIdx.x == 0) {
    t_new = set_to >= 0 ? set_to : *step - 1;
    *step = t_new;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += 256) time_in[b] = (float)(t_new + 1);
}

struct AxpbyArgs {
  const float* in[4];
  float coef[4];
  int n_in;
};

template <int V>
__global__ void __launch_bounds__(256) axpby_kernel(AxpbyArgs a, float* __restrict__ out, long nvec) {
  FOR_EACH_VEC(i, nvec) {
    float acc[V];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= a.n_in) break;
      float v[V];
      load<V>(v, a.in[k] + i * V);
      // acc = fma(c_k, v_k, acc): one rounding per term, written out so that it depends on no contraction mode.  The
      // DPM-Solver updates are built from this kernel, and their ill-conditioned fixtures sit closer to the reference with the
      // fused sum than with a product rounded on its own.
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = k == 0 ? mul_rounded(a.coef[0], v[j]) : __fmaf_rn(a.coef[k], v[j], acc[j]);
    }
    store<V>(out + i * V, acc);
  }
}

// ---- multi-tensor kernels: a list of tensors in ONE launch (the EMA update and the optimizer step of 272 parameter tensors;
// one launch per tensor cost the host 272 calls per step).  Workgroup = one chunk of at most MT_CHUNK elements of one tensor;
// chunk -> (tensor, index of the chunk within it) through two small device tables (ops.chunk_tables).
constexpr int MT_CHUNK = 16384;

// the entry and the element range [lo, hi) of this workgroup's chunk (Entry: tmdiff_mt_entry or tmdiff_adamw_entry)
template <class Entry>
struct Chunk { Entry e; long lo, hi; };
template <class Entry>
__device__ __forceinline__ Chunk<Entry> chunk_of(const Entry* __restrict__ tensors, const int32_t* __restrict__ chunk_tensor,
                                                 const int32_t* __restrict__ chunk_index) {
  const Entry e = tensors[chunk_tensor[blockIdx.x]];
  const long lo = (long)chunk_index[blockIdx.x] * MT_CHUNK;
  return {e, lo, min(lo + MT_CHUNK, (long)e.n)};
}

// THE walk over [lo, hi) by 256 lanes: vec (the tensor's pointers are 16-byte aligned; a chunk starts at a multiple of 4):
// body(Vec4, i) on four elements per lane, then body(Vec1, i) on the tail of at most three; else body(Vec1, i) throughout.
template <class F>
__device__ __forceinline__ void walk_chunk(long lo, long hi, bool vec, F&& body) {
  long i0 = lo;
  if (vec) {
    const long hi4 = lo + ((hi - lo) & ~3L);
    for (long i = lo + threadIdx.x * 4L; i < hi4; i += 1024) body(Vec4{}, i);
    i0 = hi4;
  }
  for (long i = i0 + threadIdx.x; i < hi; i += 256) body(Vec1{}, i);
}

// out_t = ca * a_t + cb * b_t (the EMA update, utils/EmaUpdater.py:23-38)
__global__ void __launch_bounds__(256) multi_axpby_kernel(const tmdiff_mt_entry* __restrict__ tensors,
                                                          const int32_t* __restrict__ chunk_tensor,
                                                          const int32_t* __restrict__ chunk_index, float ca, float cb) {
  const auto c = chunk_of(tensors, chunk_tensor, chunk_index);
  walk_chunk(c.lo, c.hi, aligned16(c.e.out) && aligned16(c.e.a) && aligned16(c.e.b), [&](auto vt, long i) {
    constexpr int V = decltype(vt)::value;
    float x[V], y[V];
    load<V>(x, c.e.a + i);
    load<V>(y, c.e.b + i);
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = __fadd_rn(mul_rounded(ca, x[j]), mul_rounded(cb, y[j]));
    store<V>(c.e.out + i, x);
  });
}

// Multi-tensor AdamW (torch.optim.AdamW semantics: decoupled weight decay, bias-corrected moments, amsgrad off) over a list of
// (parameter, gradient, exp_avg, exp_avg_sq) tensors in ONE launch -- the optimizer step of the finetune loop (reference
// GeneralModel/model.py:30-31, :43: torch.optim.AdamW(lr, weight_decay=1e-4)).  The learning rate and the step count are read
// from DEVICE scalars, so the launch can be recorded into a HIP graph and replayed (torch's own capturable path runs ~25
// multi-tensor / elementwise launches for the same update: 3 ms per step of this network against 0.15 ms here).  Operation order
// as torch's _multi_tensor_adamw: p *= 1 - lr * wd; m = lerp(m, g, 1 - b1); v = b2 v + (1 - b2) g^2;
// p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps), with bc1 = 1 - b1^t, bc2 = 1 - b2^t evaluated in double as the eager optimizer does.
struct AdamwCoef {
  float decay, w1, w2, beta2, step_size, bc2_sqrt, eps;
};

__device__ __forceinline__ AdamwCoef adamw_coef(const float* __restrict__ lr_dev, const float* __restrict__ step_dev, float beta1,
                                                float beta2, float eps, float weight_decay) {
  const float lr = *lr_dev;
  const double t = (double)*step_dev;
  const double bc1 = 1.0 - pow((double)beta1, t), bc2 = 1.0 - pow((double)beta2, t);
  return AdamwCoef{(float)(1.0 - (double)lr * (double)weight_decay), 1.f - beta1, 1.f - beta2, beta2, (float)((double)lr / bc1),
                   (float)sqrt(bc2), eps};
}

// the update of ONE element
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, const AdamwCoef& k) {
  p = mul_rounded(p, k.decay);
  m = __fadd_rn(m, mul_rounded(k.w1, __fsub_rn(g, m)));
  v = __fadd_rn(mul_rounded(v, k.beta2), mul_rounded(mul_rounded(k.w2, g), g));
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), k.bc2_sqrt), k.eps);
  p = __fsub_rn(p, mul_rounded(k.step_size, __fdiv_rn(m, denom)));
}

// One launch for the plain step and for the step on gradients scaled by *coef_dev (SCALED; global-norm clipping:
// multi_sqnorm_finish_kernel below wrote it).  The product with the gradient (one rounding) lives in registers only, the gradient
// tensor is never written.  *ok_dev == 0 (a non-finite norm) skips the step before any table read: p / m / v keep their bits.
// The plain step passes NULL for both and reads neither.
template <bool SCALED>
__global__ void __launch_bounds__(256) multi_adamw_kernel(const tmdiff_adamw_entry* __restrict__ tensors,
                                                          const int32_t* __restrict__ chunk_tensor,
                                                          const int32_t* __restrict__ chunk_index, const float* __restrict__ lr_dev,
                                                          const float* __restrict__ step_dev, float beta1, float beta2, float eps,
                                                          float weight_decay, const float* __restrict__ coef_dev,
                                                          const float* __restrict__ ok_dev) {
  if constexpr (SCALED)
    if (*ok_dev == 0.f) return;
  const auto c = chunk_of(tensors, chunk_tensor, chunk_index);
  const tmdiff_adamw_entry& e = c.e;
  const AdamwCoef k = adamw_coef(lr_dev, step_dev, beta1, beta2, eps, weight_decay);
  const float coef = SCALED ? *coef_dev : 1.f;
  walk_chunk(c.lo, c.hi, aligned16(e.p) && aligned16(e.g) && aligned16(e.m) && aligned16(e.v), [&](auto vt, long i) {
    constexpr int V = decltype(vt)::value;
    if constexpr (V == 1) {         // (in memory, as it always was: the compiler may not assume that p, m and v are distinct)
      adamw_one(e.p[i], SCALED ? mul_rounded(e.g[i], coef) : e.g[i], e.m[i], e.v[i], k);
    } else {
      float p[V], g[V], m[V], v[V];
      load<V>(p, e.p + i);
      load<V>(m, e.m + i);
      load<V>(v, e.v + i);
      load<V>(g, e.g + i);
#pragma unroll
      for (int j = 0; j < V; ++j) adamw_one(p[j], SCALED ? mul_rounded(g[j], coef) : g[j], m[j], v[j], k);
      store<V>(e.p + i, p);
      store<V>(e.m + i, m);
      store<V>(e.v + i, v);
    }
  });
}

// Global gradient norm in two stages, both without atomics and with a fixed summation order (stats.h block_sum_f64), so the
// norm has the same bits from run to run and from an eager launch to a graph replay.
// Stage 1: workgroup k sums g^2 over chunk k of the AdamW tables (same entries, same chunks) into partials[k].  Each lane adds
// the squares of its strided elements in double (the square of a float is exact there) in element order, 16 bytes per load
// where the gradient is 16-byte aligned.
__global__ void __launch_bounds__(256) multi_sqnorm_partial_kernel(const tmdiff_adamw_entry* __restrict__ tensors,
                                                                   const int32_t* __restrict__ chunk_tensor,
                                                                   const int32_t* __restrict__ chunk_index,
                                                                   double* __restrict__ partials) {
  __shared__ double red[4];
  const auto c = chunk_of(tensors, chunk_tensor, chunk_index);
  double acc = 0.0;
  walk_chunk(c.lo, c.hi, aligned16(c.e.g), [&](auto vt, long i) {
    constexpr int V = decltype(vt)::value;
    float g[V];
    load<V>(g, c.e.g + i);
#pragma unroll
    for (int j = 0; j < V; ++j) acc += (double)g[j] * (double)g[j];
  });
  const double total = tmdiff::block_sum_f64(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// Stage 2, one workgroup: the partials of every parameter group (the norm is global, as in clip_grad_norm_), strided over the
// lanes and then the same tree; norm, clip coefficient and the finite flag as three device scalars.
__global__ void __launch_bounds__(256) multi_sqnorm_finish_kernel(const double* __restrict__ partials, int n_partials, float max_norm,
                                                                  float* __restrict__ norm_dev, float* __restrict__ coef_dev,
                                                                  float* __restrict__ ok_dev) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += 256) acc += partials[i];
  const double total = tmdiff::block_sum_f64(acc, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(total);
    const bool ok = isfinite(norm);
    const float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));     // clip_grad_norm_'s coefficient, its 1e-6 included
    *norm_dev = norm;
    *coef_dev = ok ? fminf(c, 1.f) : 0.f;
    *ok_dev = ok ? 1.f : 0.f;
  }
}

template <int V>
__global__ void __launch_bounds__(256) x0_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                 float* __restrict__ x0, long nvec, float alpha, float sigma,
                                                 int is_x_start) {
  FOR_EACH_VEC(i, nvec) {
    float xv[V], mv[V], ov[V];
    load<V>(xv, x + i * V);
    load<V>(mv, m + i * V);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      // model_wrapper: x_start output -> noise  (dpm_solver_pytorch.py:304-306)
      const float eps = is_x_start ? __fdiv_rn(__fsub_rn(xv[j], mul_rounded(alpha, mv[j])), sigma) : mv[j];
      // data_prediction_fn: noise -> x0          (:451-453)
      ov[j] = __fdiv_rn(__fsub_rn(xv[j], mul_rounded(sigma, eps)), alpha);
    }
    store<V>(x0 + i * V, ov);
  }
}

template <int V>
__global__ void __launch_bounds__(256) add_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                  float* __restrict__ out, long nvec, float sign_b) {
  FOR_EACH_VEC(i, nvec) {
    float u[V], v[V];
    load<V>(u, a + i * V);
    load<V>(v, b + i * V);
#pragma unroll
    for (int j = 0; j < V; ++j) u[j] = u[j] + mul_rounded(sign_b, v[j]);
    store<V>(out + i * V, u);
  }
}

__global__ void __launch_bounds__(256) q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                       const float* __restrict__ a, float* __restrict__ out,
                                                       long n_per) {
  const int b = blockIdx.y;
  const float ab = a[b];
  const float sb = sqrtf(__fsub_rn(1.f, mul_rounded(ab, ab)));  // (1 - a**2).sqrt()
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n_per; i += 256L * gridDim.x) {
    const long o = (long)b * n_per + i;
    out[o] = __fadd_rn(mul_rounded(ab, x0[o]), mul_rounded(sb, noise[o]));
  }
}

// ---- dynamic thresholding: per-sample k-th order statistic of |x| by 4 x 8-bit radix select ------
// |x| >= 0, so the fp32 bit pattern orders like the value.  Result: s = max(lerp(v[k], v[k+1], frac), max_val)
// as torch.quantile(..., interpolation='linear'), then x = clamp(x, -s, s) / s in place.
// A sample is spread over many workgroups (one workgroup per sample was latency-bound: 0.76 ms for 2 MB):
//   4 histogram launches (8 bits each; a launch first re-derives the bucket chosen so far from the earlier
//   histograms), one launch that counts the elements <= v[k] and finds the next larger value, one that clamps.
// Workspace per sample (QW_STRIDE words, zeroed by the entry point): [0] s, [1] min above (bits), [2..3] count <= v[k]
// (64 bit), [4 + 256*p ...] histogram of pass p.
constexpr int QU = 8;               // loads in flight per thread
constexpr int QW_STRIDE = 4 + 4 * 256;

struct QArgs {
  float* x;
  unsigned* ws;
  long n, k;
  float frac, max_val;
};

// Bucket prefix / rank-in-bucket after `passes` histogram passes.  Called by all 256 threads of a workgroup (a
// one-thread scan of up to 4 x 256 words cost more than the pass itself); per pass a block-wide inclusive scan
// finds the one bin d with excl[d] <= rank < incl[d].
__device__ __forceinline__ void q_prefix(const unsigned* __restrict__ w, int passes, long k, unsigned& prefix,
                                         unsigned long long& rank) {
  __shared__ unsigned wave_tot[4];
  __shared__ unsigned sel_bin, sel_excl;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  prefix = 0;
  rank = (unsigned long long)k;
  for (int p = 0; p < passes; ++p) {
    const unsigned c = w[4 + 256 * p + tid];
    unsigned incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    unsigned base = 0;
    for (int i = 0; i < wv; ++i) base += wave_tot[i];
    incl += base;
    const unsigned excl = incl - c;
    if ((unsigned long long)excl <= rank && rank < (unsigned long long)incl) { sel_bin = tid; sel_excl = excl; }
    __syncthreads();
    prefix |= sel_bin << (24 - 8 * p);
    rank -= sel_excl;
    __syncthreads();
  }
}

template <class F>
__device__ __forceinline__ void q_for_slice(const float* __restrict__ xs, long n, F&& f) {
  const long stride = (long)gridDim.x * 256 * QU;
  for (long i0 = (long)blockIdx.x * 256 * QU; i0 < n; i0 += stride) {
    unsigned u[QU];
#pragma unroll
    for (int j = 0; j < QU; ++j) {
      const long i = i0 + j * 256L + threadIdx.x;
      u[j] = __float_as_uint(fabsf(xs[i < n ? i : n - 1]));
    }
#pragma unroll
    for (int j = 0; j < QU; ++j) f(u[j], i0 + j * 256L + threadIdx.x < n);
  }
}

__global__ void __launch_bounds__(256) quantile_hist_kernel(const QArgs a, int pass) {
  __shared__ unsigned hist[256];
  unsigned* w = a.ws + (long)blockIdx.y * QW_STRIDE;
  const float* xs = a.x + (long)blockIdx.y * a.n;
  hist[threadIdx.x] = 0;
  unsigned prefix;
  unsigned long long rank;
  q_prefix(w, pass, a.k, prefix, rank);
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned mask_hi = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
  q_for_slice(xs, a.n, [&](unsigned u, bool live) {
    if (live && (u & mask_hi) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
  });
  __syncthreads();
  if (hist[threadIdx.x]) atomicAdd(&w[4 + 256 * pass + threadIdx.x], hist[threadIdx.x]);
}

__global__ void __launch_bounds__(256) quantile_count_kernel(const QArgs a) {
  __shared__ unsigned sh_min;
  __shared__ unsigned long long sh_cnt;
  unsigned* w = a.ws + (long)blockIdx.y * QW_STRIDE;
  const float* xs = a.x + (long)blockIdx.y * a.n;
  unsigned vlo;  // exact bit pattern of the k-th smallest |x|
  unsigned long long rank;
  q_prefix(w, 4, a.k, vlo, rank);
  if (threadIdx.x == 0) { sh_min = 0x7F800000u; sh_cnt = 0; }
  __syncthreads();
  unsigned long long cnt = 0;
  unsigned vmin = 0x7F800000u;
  q_for_slice(xs, a.n, [&](unsigned u, bool live) {
    if (live) {
      if (u <= vlo) ++cnt; else vmin = u < vmin ? u : vmin;
    }
  });
  atomicAdd(&sh_cnt, cnt);
  atomicMin(&sh_min, vmin);
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(w + 2), sh_cnt);
    atomicMin(&w[1], sh_min);
  }
}

__global__ void __launch_bounds__(256) quantile_apply_kernel(const QArgs a) {
  __shared__ float sh_s;
  unsigned* w = a.ws + (long)blockIdx.y * QW_STRIDE;
  float* xs = a.x + (long)blockIdx.y * a.n;
  unsigned prefix;
  unsigned long long rank;
  q_prefix(w, 4, a.k, prefix, rank);
  if (threadIdx.x == 0) {
    const float vlo = __uint_as_float(prefix);
    // v[k+1] equals v[k] if more copies of it remain, else it is the smallest value above it
    float vhi = vlo;
    const unsigned long long cnt_le = *reinterpret_cast<const unsigned long long*>(w + 2);
    if (a.frac > 0.f && cnt_le < (unsigned long long)a.k + 2) vhi = __uint_as_float(w[1]);
    // at::lerp: w < 0.5 ? a + w*(b-a) : b - (b-a)*(1-w)
    const float diff = __fsub_rn(vhi, vlo);
    const float qv = a.frac < 0.5f ? __fadd_rn(vlo, __fmul_rn(a.frac, diff))
                                   : __fsub_rn(vhi, __fmul_rn(diff, __fsub_rn(1.f, a.frac)));
    sh_s = fmaxf(qv, a.max_val);
  }
  __syncthreads();
  const float s = sh_s;
  const long stride = (long)gridDim.x * 256 * QU;
  for (long i0 = (long)blockIdx.x * 256 * QU; i0 < a.n; i0 += stride) {
    float v[QU];
#pragma unroll
    for (int j = 0; j < QU; ++j) {
      const long i = i0 + j * 256L + threadIdx.x;
      v[j] = xs[i < a.n ? i : a.n - 1];
    }
#pragma unroll
    for (int j = 0; j < QU; ++j) {
      const long i = i0 + j * 256L + threadIdx.x;
      if (i < a.n) xs[i] = __fdiv_rn(fminf(fmaxf(v[j], -s), s), s);
    }
  }
  // every block has read w[0..3] before any block could overwrite w[0]: s goes to a separate word read by nobody here
  if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<float*>(w)[0] = s;
}

__global__ void __launch_bounds__(256) quantile_init_kernel(unsigned* ws, long words) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < words; i += 256L * gridDim.x)
    ws[i] = (i % QW_STRIDE) == 1 ? 0x7F800000u : 0u;
}

__global__ void __launch_bounds__(256) quantile_gather_s_kernel(const unsigned* ws, float* s_out, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) s_out[b] = reinterpret_cast<const float*>(ws)[(long)b * QW_STRIDE];
}

// the scalars of both AdamW entry points
int check_adamw_scalars(const char* what, float beta1, float beta2, float eps, float weight_decay) {
  TMDIFF_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && weight_decay >= 0.f,
                 "%s: betas (%g, %g) eps %g weight_decay %g", what, (double)beta1, (double)beta2, (double)eps, (double)weight_decay);
  return TMDIFF_OK;
}

}  // namespace

extern "C" int tmdiff_ddpm_step(const float* x, const float* eps, const float* noise, const float* ms, float* out,
                                float* img_out, int64_t n, float c_recip, float c_recipm1, float coef1, float coef2,
                                float sigma, int32_t clip, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(x && eps && out, "ddpm_step: NULL pointer");
  TMDIFF_REQUIRE(n >= 0, "ddpm_step: n=%ld", (long)n);
  TMDIFF_REQUIRE(noise || sigma == 0.f, "ddpm_step: noise is NULL but sigma != 0");
  TMDIFF_REQUIRE(!img_out || ms, "ddpm_step: img_out needs ms");
  if (n == 0) return TMDIFF_OK;
  const DdpmCoef k{c_recip, c_recipm1, coef1, coef2, sigma, clip};
  return launch_elementwise({x, eps, noise, ms, out, img_out}, n, "ddpm_step", [&](auto vt, int grid, long nvec) {
    ddpm_step_kernel<decltype(vt)::value><<<grid, 256, 0, as_stream(stream)>>>(x, eps, noise, ms, out, img_out, nvec, k);
  });
}

extern "C" int tmdiff_ddpm_frame_slot(int32_t t, int32_t T, int32_t frame_every) {
  return T > 0 && frame_every > 0 && t >= 0 && t < T ? ddpm_frame_slot(t, T, frame_every) : -1;
}

extern "C" int tmdiff_ddpm_step_dev(const float* x, const float* eps, const float* noise, const float* ms, float* out,
                                    float* frames, int64_t n, const int32_t* step, const float* coef, int32_t T,
                                    int32_t frame_every, int32_t clip, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(x && eps && noise && out && step && coef, "ddpm_step_dev: NULL pointer");
  TMDIFF_REQUIRE(n >= 0 && T > 0, "ddpm_step_dev: n=%ld T=%d", (long)n, T);
  TMDIFF_REQUIRE(!frames || (ms && frame_every > 0), "ddpm_step_dev: frames need ms and frame_every > 0 (got %d)", frame_every);
  if (n == 0) return TMDIFF_OK;
  return launch_elementwise({x, eps, noise, ms, out, frames}, n, "ddpm_step_dev", [&](auto vt, int grid, long nvec) {
    ddpm_step_dev_kernel<decltype(vt)::value><<<grid, 256, 0, as_stream(stream)>>>(x, eps, noise, ms, out, frames, nvec, n, step, coef,
                                                                                  T, frame_every, clip);
  });
}

extern "C" int tmdiff_sampler_tick(int32_t* step, float* time_in, int32_t B, int32_t set_to, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(step && (time_in || B == 0) && B >= 0, "sampler_tick: bad arguments");
  sampler_tick_kernel<<<1, 256, 0, as_stream(stream)>>>(step, time_in, B, set_to);
  return check_launch("sampler_tick");
}

extern "C" int tmdiff_axpby(const float* const in[4], const float coef[4], int32_t n_in, float* out, int64_t n,
                            tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(in && coef && out, "axpby: NULL pointer");
  TMDIFF_REQUIRE(n_in >= 1 && n_in <= 4 && n >= 0, "axpby: n_in=%d n=%ld", n_in, (long)n);
  AxpbyArgs a;
  for (int k = 0; k < 4; ++k) {
    a.in[k] = k < n_in ? in[k] : nullptr;       // (a NULL operand does not count for the alignment)
    a.coef[k] = k < n_in ? coef[k] : 0.f;
    TMDIFF_REQUIRE(k >= n_in || in[k] != nullptr, "axpby: input %d is NULL", k);
  }
  a.n_in = n_in;
  if (n == 0) return TMDIFF_OK;
  return launch_elementwise({a.in[0], a.in[1], a.in[2], a.in[3], out}, n, "axpby", [&](auto vt, int grid, long nvec) {
    axpby_kernel<decltype(vt)::value><<<grid, 256, 0, as_stream(stream)>>>(a, out, nvec);
  });
}

extern "C" int32_t tmdiff_multi_axpby_chunk(void) { return MT_CHUNK; }

extern "C" int tmdiff_multi_axpby(const tmdiff_mt_entry* tensors_dev, const int32_t* chunk_tensor_dev,
                                  const int32_t* chunk_index_dev, int32_t n_chunks, float ca, float cb,
                                  tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(tensors_dev && chunk_tensor_dev && chunk_index_dev && n_chunks >= 0, "multi_axpby: bad arguments");
  if (n_chunks == 0) return TMDIFF_OK;
  multi_axpby_kernel<<<(unsigned)n_chunks, 256, 0, as_stream(stream)>>>(tensors_dev, chunk_tensor_dev, chunk_index_dev, ca, cb);
  return check_launch("multi_axpby");
}

extern "C" int tmdiff_multi_adamw(const tmdiff_adamw_entry* tensors_dev, const int32_t* chunk_tensor_dev,
                                  const int32_t* chunk_index_dev, int32_t n_chunks, const float* lr_dev, const float* step_dev,
                                  float beta1, float beta2, float eps, float weight_decay, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(tensors_dev && chunk_tensor_dev && chunk_index_dev && lr_dev && step_dev && n_chunks >= 0, "multi_adamw: bad arguments");
  if (const int rc = check_adamw_scalars("multi_adamw", beta1, beta2, eps, weight_decay)) return rc;
  if (n_chunks == 0) return TMDIFF_OK;
  multi_adamw_kernel<false><<<(unsigned)n_chunks, 256, 0, as_stream(stream)>>>(
      tensors_dev, chunk_tensor_dev, chunk_index_dev, lr_dev, step_dev, beta1, beta2, eps, weight_decay, nullptr, nullptr);
  return check_launch("multi_adamw");
}

extern "C" int tmdiff_multi_adamw_scaled(const tmdiff_adamw_entry* tensors_dev, const int32_t* chunk_tensor_dev,
                                         const int32_t* chunk_index_dev, int32_t n_chunks, const float* lr_dev,
                                         const float* step_dev, float beta1, float beta2, float eps, float weight_decay,
                                         const float* coef_dev, const float* ok_dev, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(tensors_dev && chunk_tensor_dev && chunk_index_dev && lr_dev && step_dev && coef_dev && ok_dev && n_chunks > 0,
                 "multi_adamw_scaled: bad arguments");
  if (const int rc = check_adamw_scalars("multi_adamw_scaled", beta1, beta2, eps, weight_decay)) return rc;
  multi_adamw_kernel<true><<<(unsigned)n_chunks, 256, 0, as_stream(stream)>>>(
      tensors_dev, chunk_tensor_dev, chunk_index_dev, lr_dev, step_dev, beta1, beta2, eps, weight_decay, coef_dev, ok_dev);
  return check_launch("multi_adamw_scaled");
}

extern "C" size_t tmdiff_multi_sqnorm_workspace_bytes(int32_t n_chunks) {
  return n_chunks > 0 ? (size_t)n_chunks * sizeof(double) : 0;
}

extern "C" int tmdiff_multi_sqnorm_partial(const tmdiff_adamw_entry* tensors_dev, const int32_t* chunk_tensor_dev,
                                           const int32_t* chunk_index_dev, int32_t n_chunks, double* partials_dev,
                                           tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(tensors_dev && chunk_tensor_dev && chunk_index_dev && partials_dev && n_chunks > 0,
                 "multi_sqnorm_partial: bad arguments");
  multi_sqnorm_partial_kernel<<<(unsigned)n_chunks, 256, 0, as_stream(stream)>>>(tensors_dev, chunk_tensor_dev, chunk_index_dev,
                                                                                 partials_dev);
  return check_launch("multi_sqnorm_partial");
}

extern "C" int tmdiff_multi_sqnorm_finish(const double* partials_dev, int32_t n_partials, float max_norm, float* norm_dev,
                                          float* coef_dev, float* ok_dev, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(partials_dev && norm_dev && coef_dev && ok_dev && n_partials > 0, "multi_sqnorm_finish: bad arguments");
  TMDIFF_REQUIRE(max_norm > 0.f, "multi_sqnorm_finish: max_norm %g (must be > 0)", (double)max_norm);
  multi_sqnorm_finish_kernel<<<1, 256, 0, as_stream(stream)>>>(partials_dev, n_partials, max_norm, norm_dev, coef_dev, ok_dev);
  return check_launch("multi_sqnorm_finish");
}

extern "C" int tmdiff_x0_from_model(const float* x, const float* model_out, float* x0, int64_t n, float alpha,
                                    float sigma, int32_t model_is_x_start, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(x && model_out && x0 && n >= 0, "x0_from_model: bad arguments");
  if (n == 0) return TMDIFF_OK;
  return launch_elementwise({x, model_out, x0}, n, "x0_from_model", [&](auto vt, int grid, long nvec) {
    x0_kernel<decltype(vt)::value><<<grid, 256, 0, as_stream(stream)>>>(x, model_out, x0, nvec, alpha, sigma, model_is_x_start);
  });
}

extern "C" size_t tmdiff_abs_quantile_workspace_bytes(int32_t B, int64_t /*n_per_sample*/) {
  // [0, B) floats: the per-sample thresholds s (readable by the caller); then the select state of every sample
  return B > 0 ? ((size_t)(B + 3) / 4 * 4 + (size_t)B * QW_STRIDE) * sizeof(float) : 0;
}

extern "C" int tmdiff_abs_quantile_clamp(float* x0, int32_t B, int64_t n_per_sample, float q, float max_val,
                                         void* workspace, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(x0 && workspace && B >= 0 && n_per_sample > 0, "abs_quantile_clamp: bad arguments");
  TMDIFF_REQUIRE(q >= 0.f && q <= 1.f, "abs_quantile_clamp: q=%f outside [0,1]", q);
  TMDIFF_REQUIRE(B <= 65535, "abs_quantile_clamp: B=%d", B);
  if (B == 0) return TMDIFF_OK;
  // torch.quantile: rank = q * (n - 1) evaluated in the input dtype (fp32); lerp weight = rank - floor(rank)
  const float rank = q * (float)(n_per_sample - 1);
  long k = (long)floorf(rank);
  if (k > n_per_sample - 1) k = n_per_sample - 1;
  float* s_out = reinterpret_cast<float*>(workspace);
  QArgs a{x0, reinterpret_cast<unsigned*>(workspace) + (B + 3) / 4 * 4, n_per_sample, k, rank - (float)k, max_val};
  hipStream_t st = as_stream(stream);
  long per = (n_per_sample + 256 * QU - 1) / (256 * QU);  // workgroups per sample: one batch of loads each, capped
  const long cap = B >= 256 ? 4 : 1024 / B;
  if (per > cap) per = cap;
  const dim3 grid((unsigned)per, (unsigned)B);
  const long words = (long)B * QW_STRIDE;
  quantile_init_kernel<<<(unsigned)((words + 255) / 256), 256, 0, st>>>(a.ws, words);
  for (int pass = 0; pass < 4; ++pass) quantile_hist_kernel<<<grid, 256, 0, st>>>(a, pass);
  quantile_count_kernel<<<grid, 256, 0, st>>>(a);
  quantile_apply_kernel<<<grid, 256, 0, st>>>(a);
  quantile_gather_s_kernel<<<(B + 255) / 256, 256, 0, st>>>(a.ws, s_out, B);
  return check_launch("abs_quantile_clamp");
}

extern "C" int tmdiff_add(const float* a, const float* b, float* out, int64_t n, float sign_b, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(a && b && out && n >= 0, "add: bad arguments");
  if (n == 0) return TMDIFF_OK;
  return launch_elementwise({a, b, out}, n, "add", [&](auto vt, int grid, long nvec) {
    add_kernel<decltype(vt)::value><<<grid, 256, 0, as_stream(stream)>>>(a, b, out, nvec, sign_b);
  });
}

extern "C" int tmdiff_q_sample(const float* x0, const float* noise, const float* a, float* out, int32_t B,
                               int64_t n_per_sample, tmdiff_stream_t stream) {
  using namespace tmdiff;
  TMDIFF_REQUIRE(x0 && noise && a && out && B >= 0 && B <= 65535 && n_per_sample >= 0, "q_sample: bad arguments");
  if (B == 0 || n_per_sample == 0) return TMDIFF_OK;
  long blocks = (n_per_sample + 255) / 256;
  if (blocks > 256) blocks = 256;
  q_sample_kernel<<<dim3((unsigned)blocks, B), 256, 0, as_stream(stream)>>>(x0, noise, a, out, n_per_sample);
  return check_launch("q_sample");
}

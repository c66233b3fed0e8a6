// The SSIM finetune loss term with its gradient (gfx950; host definition: tmdiff_amd/losses.py ssim_loss_host):
//
//   dssim = 1 - SSIM(x_true, x_pred)                 fp32 [B, C, H, W] tensors; x_true = x0 (+ ms), x_pred = xh (+ ms)
//
//  SSIM  the mean over all B C (H - win + 1)(W - win + 1) windows of S = (A1 A2) / (B1 B2): a uniform win x win window per band
//        plane, 'valid', n = win^2, k = n / (n - 1), f = the window mean,
//          ux = f(a), uy = f(b), vx = k (f(a a) - ux^2), vy = k (f(b b) - uy^2), vxy = k (f(a b) - ux uy),
//          A1 = 2 ux uy + c1, A2 = 2 vxy + c2, B1 = ux^2 + uy^2 + c1, B2 = vx + vy + c2, c1 = (0.01 R)^2, c2 = (0.03 R)^2.
//        (metrics.ssim's definition.)  Its gradient with respect to b = x_pred, from three per-window maps
//          Q = 2 k A1 / (B1 B2),  R = -k S / B2,  P = 2 ux A2 / (B1 B2) - 2 k ux A1 / (B1 B2) - 2 uy S / B1 + 2 k uy S / B2:
//          d dssim / d b[p] = -(1 / (n Nwin)) (sum P + a[p] sum Q + 2 b[p] sum R), the sums over the windows that contain p.
//
//  TILE: 16 x 32 pixels of one band plane per workgroup of 256 lanes (TH, TW below), for every window size.
//
//  ssim_loss_kernel     stages a and b of the tile with a halo of win - 1 rows and of win - 1 columns rounded up to a multiple of
//                       4 (so that a float4 lies inside the image or outside it) in LDS: as floats, or as the fp64 sums with ms
//                       when ms is given.  A lane then owns four neighbouring windows of a row and forms their five sums directly
//                       (f(a b), f(a a) and f(b b) by one fma sequence: a == b gives S == 1 exactly), for every window that
//                       contains a tile pixel: origins from tile - (win - 1).  The windows whose origin lies in the tile count in
//                       the value sum.  P, Q, R go to LDS (0 for an origin outside the valid region), and a lane sums them
//                       directly over the win x win windows around each of its four pixels.  g == NULL: values only, and only the
//                       windows of the value sum are formed.  accumulate: g = fl32(g + ...), else g = fl32(...).
//  ssim_finalize_kernel adds the workgroups' partial sums (stats.h strided_sum, block_sum_f64) and writes the values (alone, or
//                       composed with the four values of csrc/loss.hip).
//
// Every operation after the fp32 loads is fp64.  No atomics: one partial sum per workgroup (stats.h block_sum_f64) goes to the
// workspace with a plain vector store, so a call is reproducible bit for bit; nothing is allocated, copied or synchronised here.
#include <cfloat>
#include <type_traits>

#include "stats.h"

namespace {

constexpr int TH = 16, TW = 32, NT = 256, FIN_T = 256;

template <int WIN>
struct Geo {
  static constexpr int HALO = WIN - 1, PADX = (HALO + 3) / 4 * 4;   // rows / columns staged around the tile
  static constexpr int LH = TH + 2 * HALO, LS = TW + 2 * PADX;      // staged tile; column x0 - PADX + lx
  static constexpr int MH = TH + HALO, MW = TW + PADX;              // window origins (y0 - HALO + my, x0 - PADX + mx)
  static constexpr int NSTRIP = MW / 4, NV = WIN + 3;               // strips of four windows; staged values a strip's row reads
};

inline long tiles_of(int H, int W) { return (long)((H + TH - 1) / TH) * ((W + TW - 1) / TW); }

struct SsimArgs {
  const float* xt;
  const float* xp;
  const float* ms;   // null: x_true = xt, x_pred = xp
  float* g;          // null: values only
  int H, W, tiles_x, tiles, vec, accumulate;
  double c1, c2;
  double gscale;     // -weight / (n Nwin)
  double* part;      // [workgroups]: sum of S over the windows whose origin lies in the tile
};

// S and the three maps of one window from its five sums.  Every operation is rounded on its own, and the expressions in a and b
// are written alike: equal sums give A1 == B1 and A2 == B2 bit for bit.
__device__ __forceinline__ void window_maps(double fa, double fb, double faa, double fbb, double fab, double inv_n, double k,
                                            double c1, double c2, double& S, double& P, double& Q, double& R) {
#pragma clang fp contract(off)
  const double ux = fa * inv_n, uy = fb * inv_n;
  const double vx = k * (faa * inv_n - ux * ux), vy = k * (fbb * inv_n - uy * uy), vxy = k * (fab * inv_n - ux * uy);
  const double A1 = 2.0 * ux * uy + c1, A2 = 2.0 * vxy + c2, B1 = ux * ux + uy * uy + c1, B2 = vx + vy + c2;
  S = (A1 * A2) / (B1 * B2);
  const double r1 = 1.0 / B1, r2 = 1.0 / B2, rd = r1 * r2;
  Q = 2.0 * k * A1 * rd;
  R = -k * S * r2;
  P = 2.0 * ux * A2 * rd - 2.0 * k * ux * A1 * rd - 2.0 * uy * S * r1 + 2.0 * k * uy * S * r2;
}

template <int WIN, class T>
__global__ void __launch_bounds__(NT) ssim_loss_kernel(SsimArgs p) {
  using G = Geo<WIN>;
  constexpr bool MS = std::is_same<T, double>::value;
  __shared__ __attribute__((aligned(16))) T sa[G::LH * G::LS];   // x_true
  __shared__ __attribute__((aligned(16))) T sb[G::LH * G::LS];   // x_pred
  __shared__ __attribute__((aligned(16))) double mp[G::MH * G::MW], mq[G::MH * G::MW], mr[G::MH * G::MW];
  __shared__ double red[NT / 64];

  const int t = threadIdx.x;
  const int pl = blockIdx.x / p.tiles, tile = blockIdx.x - pl * p.tiles;
  const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
  const int y0 = ty * TH, x0 = tx * TW;
  const int H = p.H, W = p.W;
  const long pbase = (long)pl * H * W;
  const float* pa = p.xt + pbase;
  const float* pb = p.xp + pbase;
  const float* pm = MS ? p.ms + pbase : nullptr;

  tmdiff::stage_halo_tile<T, G::LH, G::LS, G::LS, NT>(sa, sb, pa, pb, pm, y0 - G::HALO, x0 - G::PADX, H, W, p.vec != 0);
  __syncthreads();

  constexpr int n = WIN * WIN;
  const double inv_n = 1.0 / n, k = (double)n / (n - 1);
  const bool want_g = p.g != nullptr;
  double s_val = 0.0;
  for (int s = t; s < G::MH * G::NSTRIP; s += NT) {
    const int my = s / G::NSTRIP, mx = 4 * (s - my * G::NSTRIP);
    const int oy = y0 - G::HALO + my, ox = x0 - G::PADX + mx;          // origin of the strip's first window
    const bool row_ok = oy >= 0 && oy <= H - WIN;
    const bool own_row = my >= G::HALO;                                 // origins inside the tile count in the value
    bool any = row_ok && ox + 3 >= 0 && ox <= W - WIN;
    if (!want_g) any = any && own_row && mx + 3 >= G::PADX;
    double P[4] = {0.0, 0.0, 0.0, 0.0}, Q[4] = {0.0, 0.0, 0.0, 0.0}, R[4] = {0.0, 0.0, 0.0, 0.0};
    if (any) {
      double fa[4] = {0.0, 0.0, 0.0, 0.0}, fb[4] = {0.0, 0.0, 0.0, 0.0}, faa[4] = {0.0, 0.0, 0.0, 0.0},
             fbb[4] = {0.0, 0.0, 0.0, 0.0}, fab[4] = {0.0, 0.0, 0.0, 0.0};
      for (int dy = 0; dy < WIN; ++dy) {
        const T* ra = &sa[(my + dy) * G::LS + mx];
        const T* rb = &sb[(my + dy) * G::LS + mx];
        double a[G::NV], b[G::NV];
#pragma unroll
        for (int j = 0; j < G::NV; ++j) a[j] = (double)ra[j], b[j] = (double)rb[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int dx = 0; dx < WIN; ++dx) {
            const double u = a[j + dx], v = b[j + dx];
            fa[j] += u; fb[j] += v;
            faa[j] = fma(u, u, faa[j]); fbb[j] = fma(v, v, fbb[j]); fab[j] = fma(u, v, fab[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (ox + j >= 0 && ox + j <= W - WIN) {
          double S;
          window_maps(fa[j], fb[j], faa[j], fbb[j], fab[j], inv_n, k, p.c1, p.c2, S, P[j], Q[j], R[j]);
          if (own_row && mx + j >= G::PADX) s_val += S;
        }
      }
    }
    if (want_g) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        mp[my * G::MW + mx + j] = P[j]; mq[my * G::MW + mx + j] = Q[j]; mr[my * G::MW + mx + j] = R[j];
      }
    }
  }

  if (want_g) {
    __syncthreads();
    for (int s = t; s < TH * (TW / 4); s += NT) {
      const int row = s / (TW / 4), lx = 4 * (s - row * (TW / 4));
      const int gy = y0 + row, gx = x0 + lx;
      if (gy >= H || gx >= W) continue;
      double sp[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0}, sr[4] = {0.0, 0.0, 0.0, 0.0};
      for (int dy = 0; dy < WIN; ++dy) {          // the windows that contain pixel (row, lx + j): origins (row .. + HALO, lx + j + PADX - HALO .. + HALO)
        const int o = (row + dy) * G::MW + lx + G::PADX - G::HALO;
        double vp[G::NV], vq[G::NV], vr[G::NV];
#pragma unroll
        for (int j = 0; j < G::NV; ++j) vp[j] = mp[o + j], vq[j] = mq[o + j], vr[j] = mr[o + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int dx = 0; dx < WIN; ++dx) sp[j] += vp[j + dx], sq[j] += vq[j + dx], sr[j] += vr[j + dx];
        }
      }
      const int c = (row + G::HALO) * G::LS + G::PADX + lx;
      double d[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = p.gscale * (sp[j] + (double)sa[c + j] * sq[j] + 2.0 * (double)sb[c + j] * sr[j]);
      float* pg = p.g + pbase + (long)gy * W + gx;
      if (p.vec) {
        float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.accumulate) o4 = *reinterpret_cast<const float4*>(pg);
        o4.x = (float)((double)o4.x + d[0]); o4.y = (float)((double)o4.y + d[1]);
        o4.z = (float)((double)o4.z + d[2]); o4.w = (float)((double)o4.w + d[3]);
        *reinterpret_cast<float4*>(pg) = o4;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (gx + j < W) {
            const float old = p.accumulate ? pg[j] : 0.f;
            pg[j] = (float)((double)old + d[j]);
          }
        }
      }
    }
  }

  const double w = tmdiff::block_sum_f64(s_val, red);
  if (t == 0) p.part[blockIdx.x] = w;
}

struct SsimFinalArgs {
  const double* part;
  long n;                   // workgroups
  double nwin, weight;
  const double* terms_in;   // null, or the four values of csrc/loss.hip
  double* out64;            // [2] = dssim, ssim; with terms_in [5] = total, base, sam, lap, dssim
  float* out32;             // weight * dssim; with terms_in the total
};

// Lane t adds the workgroups t, t + 256, ... in order, then the workgroup sum: the order depends on the number of workgroups alone.
__global__ void __launch_bounds__(FIN_T) ssim_finalize_kernel(SsimFinalArgs p) {
  __shared__ double red[FIN_T / 64];
  const double tot = tmdiff::block_sum_f64(tmdiff::strided_sum(p.part, p.n, 1, threadIdx.x, FIN_T), red);
  if (threadIdx.x != 0) return;
  const double ssim = tot / p.nwin, dssim = 1.0 - ssim;
  if (p.terms_in) {
#pragma clang fp contract(off)   // terms_in[0] + weight * dssim with both operations rounded, as the host writes it
    const double t0 = p.terms_in[0], t1 = p.terms_in[1], t2 = p.terms_in[2], t3 = p.terms_in[3];
    const double total = t0 + p.weight * dssim;
    p.out64[0] = total; p.out64[1] = t1; p.out64[2] = t2; p.out64[3] = t3; p.out64[4] = dssim;
    *p.out32 = (float)total;
  } else {
    p.out64[0] = dssim; p.out64[1] = ssim;
    *p.out32 = (float)(p.weight * dssim);
  }
}

bool ssim_ok(int B, int C, int H, int W, int win) {
  return B >= 1 && C >= 1 && win >= 3 && win <= 11 && (win & 1) && H >= win && W >= win && tmdiff::fits_int32((double)B * C * H * W);
}

size_t ssim_bytes(int B, int C, int H, int W) { return (size_t)B * C * tiles_of(H, W) * sizeof(double); }

template <int WIN>
void launch(const SsimArgs& a, unsigned blocks, hipStream_t st) {
  if (a.ms) ssim_loss_kernel<WIN, double><<<blocks, NT, 0, st>>>(a);
  else ssim_loss_kernel<WIN, float><<<blocks, NT, 0, st>>>(a);
}

}  // namespace

extern "C" {

int tmdiff_ssim_loss_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t win) {
  return ssim_ok(B, C, H, W, win);   // a predicate: it leaves the last-error string alone
}

size_t tmdiff_ssim_loss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t win) {
  return ssim_ok(B, C, H, W, win) ? ssim_bytes(B, C, H, W) : 0;
}

int tmdiff_ssim_loss(const float* x_true, const float* x_pred, const float* ms, float* g, int32_t win, double data_range,
                     double weight, int32_t accumulate, const double* terms_in, double* out64, float* out32, void* workspace,
                     size_t workspace_bytes, int32_t B, int32_t C, int32_t H, int32_t W, tmdiff_stream_t stream) {
  if (!ssim_ok(B, C, H, W, win))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "ssim_loss: B=%d C=%d H=%d W=%d win=%d (B, C >= 1, odd 3 <= win <= 11, H, W >= win, "
                        "fewer than 2^31 elements)", B, C, H, W, win);
  if (!(data_range > 0.0 && data_range <= DBL_MAX && weight >= 0.0 && weight <= DBL_MAX))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "ssim_loss: data_range=%g weight=%g (data_range > 0, weight >= 0, both finite)",
                        data_range, weight);
  TMDIFF_REQUIRE(x_true && x_pred && out64 && out32 && workspace, "ssim_loss: null tensor");
  TMDIFF_REQUIRE(g || !accumulate, "ssim_loss: accumulate needs a gradient tensor");
  if (const int rc = tmdiff::check_workspace("ssim_loss", workspace, workspace_bytes, ssim_bytes(B, C, H, W), ", as out64 and terms_in",
                                             out64, terms_in))
    return rc;
  const hipStream_t st = tmdiff::as_stream(stream);
  const long tiles = tiles_of(H, W), blocks = (long)B * C * tiles;
  if (const int rc = tmdiff::check_grid(blocks, "ssim_loss", TMDIFF_E_UNSUPPORTED)) return rc;
  const bool vec = W % 4 == 0 && tmdiff::aligned16(x_true) && tmdiff::aligned16(x_pred) && (!ms || tmdiff::aligned16(ms)) &&
                   (!g || tmdiff::aligned16(g));
  const double nwin = (double)B * C * (H - win + 1) * (W - win + 1), r1 = 0.01 * data_range, r2 = 0.03 * data_range;
  const SsimArgs a{x_true, x_pred, ms, g, H, W, (W + TW - 1) / TW, (int)tiles, vec, accumulate != 0, r1 * r1, r2 * r2,
                   -weight / ((double)(win * win) * nwin), static_cast<double*>(workspace)};
  switch (win) {
    case 3: launch<3>(a, (unsigned)blocks, st); break;
    case 5: launch<5>(a, (unsigned)blocks, st); break;
    case 7: launch<7>(a, (unsigned)blocks, st); break;
    case 9: launch<9>(a, (unsigned)blocks, st); break;
    default: launch<11>(a, (unsigned)blocks, st); break;
  }
  if (const int rc = tmdiff::check_launch("ssim_loss")) return rc;
  const SsimFinalArgs f{a.part, blocks, nwin, weight, terms_in, out64, out32};
  ssim_finalize_kernel<<<1, FIN_T, 0, st>>>(f);
  return tmdiff::check_launch("ssim_loss (finalize)");
}

}  // extern "C"

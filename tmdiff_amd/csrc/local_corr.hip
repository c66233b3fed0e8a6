// The local PAN-correlation loss with its gradient (gfx950; host definition: tmdiff_amd/metrics.py local_corr_loss):
//
//   loss = mean over b, c and windows of max(0, rho_max[c] - rho),   D_rho = 1 - mean rho
//
//  rho   the correlation coefficient of band c of x [B, C, H, W] and pan [B, 1, H, W] inside a win x win window, every window at
//        stride 1, 'valid': (H - win + 1)(W - win + 1) windows per plane, n = win^2.  Two-pass centred sums: first the window
//        means mx = sum(x) / n and mp = sum(p) / n (true divisions: n v / n == v for fp32 v and n <= 64), then with u = x - mx and
//        v = p - mp the sums S_xx = sum u u, S_pp = sum v v, S_xp = sum u v, and
//          rho = S_xp / sqrt(S_xx S_pp),   0 where S_xx S_pp == 0 exactly.  No eps anywhere.
//        A window is ACTIVE iff rho < rho_max[c].  The gradient with respect to x, from three per-window maps with
//        w = -weight / N on active windows with S_xx S_pp != 0 and 0 elsewhere (N: all B C (H - win + 1)(W - win + 1) windows):
//          a = w / sqrt(S_xx S_pp),  b = -w rho / S_xx,  c = -(a mp + b mx):
//          g[k] = p[k] sum a + x[k] sum b + sum c, the sums over the windows that contain k.  pan gets no gradient.
//
//  TILE: 16 x 32 pixels per workgroup of 256 lanes (TH, TW below), for every window size 2 .. 8.
//
//  local_corr_kernel    one workgroup per (image, tile).  The PAN tile with a halo of win - 1 rows and of win - 1 columns rounded
//                       up to a multiple of 4 is staged in LDS once; a lane owns one strip of four neighbouring windows of a row
//                       (there are at most 256 strips for win <= 8) and keeps their mp and S_pp in registers.  Then, band by band:
//                       the band's tile is staged, the lane forms mx, S_xx, S_xp and rho of its four windows, adds the windows
//                       whose origin lies in the tile to its two value sums (rho, hinge) and writes a, b, c to LDS (0 for an
//                       origin outside the valid region); after a barrier a lane sums the maps over the win x win windows around
//                       each of its four pixels (the adjoint box filter) and stores g, rounded to fp32 once.  g == NULL: values
//                       only, and only the windows of the value sums are formed.  accumulate: g = fl32(g + ...).
//  local_corr_finalize  adds the workgroups' partial sums image by image (stats.h strided_sum, block_sum_f64: the order inside an
//                       image depends on the tile count alone, so a batch reports what its samples report), then the images in
//                       ascending order, and writes the values.
//
// Every operation after the fp32 loads is fp64.  No atomics: two partial sums per workgroup go to the workspace with plain vector
// stores, so a call is reproducible bit for bit; nothing is allocated, copied or synchronised here.
#include <cfloat>

#include "stats.h"

namespace {

constexpr int TH = 16, TW = 32, NT = 256, FIN_T = 256;

template <int WIN>
struct Geo {
  static constexpr int HALO = WIN - 1, PADX = (HALO + 3) / 4 * 4;   // rows / columns staged around the tile
  static constexpr int LH = TH + 2 * HALO, LS = TW + 2 * PADX;      // staged tile; column x0 - PADX + lx
  static constexpr int MH = TH + HALO, MW = TW + PADX;              // window origins (y0 - HALO + my, x0 - PADX + mx)
  static constexpr int NSTRIP = MW / 4, NV = WIN + 3;               // strips of four windows; staged values a strip's row reads
  static_assert(MH * NSTRIP <= NT, "a lane owns one strip: its PAN sums stay in registers over the bands");
};

inline long tiles_of(int H, int W) { return (long)((H + TH - 1) / TH) * ((W + TW - 1) / TW); }

struct LcorrArgs {
  const float* x;
  const float* pan;
  float* g;               // null: values only
  const double* rho_max;  // [C], or null: 1.0 for every band
  int C, H, W, tiles_x, tiles, vec, accumulate;
  double w;               // -weight / N
  double* part;           // [B * tiles][2]: sums of rho and of the hinge over the windows whose origin lies in the tile, all bands
};

// Rows yy0 .. yy0 + LH - 1 and columns xx0 .. xx0 + LS - 1 of the H x W plane src into dst (row stride LS), zero outside the
// image.  `vec`: 16-byte loads (W % 4 == 0, the plane 16-byte aligned; xx0 and LS are multiples of 4, so four columns lie inside
// the image or outside it together).  Otherwise scalar loads, where a lane outside the image reads element (0, 0).
template <int LH, int LS>
__device__ __forceinline__ void stage_plane(float* dst, const float* src, int yy0, int xx0, int H, int W, bool vec) {
  static_assert(LS % 4 == 0, "float4 rows");
  if (vec) {
    for (int i = threadIdx.x; i < LH * (LS / 4); i += NT) {
      const int ly = i / (LS / 4), lq = i - ly * (LS / 4);
      const int yy = yy0 + ly, xx = xx0 + 4 * lq;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = *reinterpret_cast<const float4*>(src + yy * W + xx);
      *reinterpret_cast<float4*>(dst + ly * LS + 4 * lq) = v;
    }
  } else {
    for (int i = threadIdx.x; i < LH * LS; i += NT) {
      const int ly = i / LS, lx = i - ly * LS;
      const int yy = yy0 + ly, xx = xx0 + lx;
      const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
      const float v = src[in ? yy * W + xx : 0];
      dst[i] = in ? v : 0.f;
    }
  }
}

template <int WIN>
__global__ void __launch_bounds__(NT) local_corr_kernel(LcorrArgs p) {
  using G = Geo<WIN>;
  __shared__ __attribute__((aligned(16))) float sp[G::LH * G::LS];   // pan
  __shared__ __attribute__((aligned(16))) float sx[G::LH * G::LS];   // the band
  __shared__ __attribute__((aligned(16))) double ma[G::MH * G::MW], mb[G::MH * G::MW], mc[G::MH * G::MW];
  __shared__ double red[(NT / 64) * 2];

  const int t = threadIdx.x;
  const int img = blockIdx.x / p.tiles, tile = blockIdx.x - img * p.tiles;
  const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
  const int y0 = ty * TH, x0 = tx * TW;
  const int H = p.H, W = p.W;
  const long plane = (long)H * W;
  const bool want_g = p.g != nullptr;
  constexpr double n = WIN * WIN;

  stage_plane<G::LH, G::LS>(sp, p.pan + img * plane, y0 - G::HALO, x0 - G::PADX, H, W, p.vec != 0);

  // the lane's strip: four windows with origins (oy, ox .. ox + 3)
  const bool has_strip = t < G::MH * G::NSTRIP;
  const int my = has_strip ? t / G::NSTRIP : 0, mx = has_strip ? 4 * (t - my * G::NSTRIP) : 0;
  const int oy = y0 - G::HALO + my, ox = x0 - G::PADX + mx;
  const bool own_row = my >= G::HALO;                                  // origins inside the tile count in the values
  bool any = has_strip && oy >= 0 && oy <= H - WIN && ox + 3 >= 0 && ox <= W - WIN;
  if (!want_g) any = any && own_row && mx + 3 >= G::PADX;
  bool valid[4], own[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    valid[j] = any && ox + j >= 0 && ox + j <= W - WIN;
    own[j] = valid[j] && own_row && mx + j >= G::PADX;
  }
  __syncthreads();

  double mp[4] = {0.0, 0.0, 0.0, 0.0}, spp[4] = {0.0, 0.0, 0.0, 0.0};
  if (any) {
    for (int dy = 0; dy < WIN; ++dy) {
      const float* rp = &sp[(my + dy) * G::LS + mx];
      double v[G::NV];
#pragma unroll
      for (int j = 0; j < G::NV; ++j) v[j] = (double)rp[j];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int dx = 0; dx < WIN; ++dx) mp[j] += v[j + dx];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) mp[j] = mp[j] / n;
    for (int dy = 0; dy < WIN; ++dy) {
      const float* rp = &sp[(my + dy) * G::LS + mx];
      double v[G::NV];
#pragma unroll
      for (int j = 0; j < G::NV; ++j) v[j] = (double)rp[j];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int dx = 0; dx < WIN; ++dx) {
          const double d = v[j + dx] - mp[j];
          spp[j] = fma(d, d, spp[j]);
        }
      }
    }
  }

  double s_rho = 0.0, s_hinge = 0.0;
  for (int c = 0; c < p.C; ++c) {
    const long pbase = ((long)img * p.C + c) * plane;
    const double rmax = p.rho_max ? p.rho_max[c] : 1.0;
    if (c > 0) __syncthreads();                                        // the gather of band c - 1 has read sx and the maps
    stage_plane<G::LH, G::LS>(sx, p.x + pbase, y0 - G::HALO, x0 - G::PADX, H, W, p.vec != 0);
    __syncthreads();

    double A[4] = {0.0, 0.0, 0.0, 0.0}, Bm[4] = {0.0, 0.0, 0.0, 0.0}, Cm[4] = {0.0, 0.0, 0.0, 0.0};
    if (any) {
      double mxv[4] = {0.0, 0.0, 0.0, 0.0}, sxx[4] = {0.0, 0.0, 0.0, 0.0}, sxp[4] = {0.0, 0.0, 0.0, 0.0};
      for (int dy = 0; dy < WIN; ++dy) {
        const float* rx = &sx[(my + dy) * G::LS + mx];
        double u[G::NV];
#pragma unroll
        for (int j = 0; j < G::NV; ++j) u[j] = (double)rx[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int dx = 0; dx < WIN; ++dx) mxv[j] += u[j + dx];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) mxv[j] = mxv[j] / n;
      for (int dy = 0; dy < WIN; ++dy) {
        const float* rx = &sx[(my + dy) * G::LS + mx];
        const float* rp = &sp[(my + dy) * G::LS + mx];
        double u[G::NV], v[G::NV];
#pragma unroll
        for (int j = 0; j < G::NV; ++j) u[j] = (double)rx[j], v[j] = (double)rp[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int dx = 0; dx < WIN; ++dx) {
            const double du = u[j + dx] - mxv[j], dv = v[j + dx] - mp[j];
            sxx[j] = fma(du, du, sxx[j]);
            sxp[j] = fma(du, dv, sxp[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!valid[j]) continue;
        const double den2 = sxx[j] * spp[j];
        const bool flat = den2 == 0.0;
        const double den = sqrt(den2);
        const double rho = flat ? 0.0 : sxp[j] / den;
        const bool active = rho < rmax;
        if (own[j]) {
          s_rho += rho;
          s_hinge += active ? rmax - rho : 0.0;
        }
        if (want_g && active && !flat) {
          A[j] = p.w / den;
          Bm[j] = -(p.w * rho) / sxx[j];
          Cm[j] = -(A[j] * mp[j] + Bm[j] * mxv[j]);
        }
      }
    }
    if (want_g) {
      if (has_strip) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ma[my * G::MW + mx + j] = A[j]; mb[my * G::MW + mx + j] = Bm[j]; mc[my * G::MW + mx + j] = Cm[j];
        }
      }
      __syncthreads();
      for (int s = t; s < TH * (TW / 4); s += NT) {
        const int row = s / (TW / 4), lx = 4 * (s - row * (TW / 4));
        const int gy = y0 + row, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        double sa[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0}, sc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int dy = 0; dy < WIN; ++dy) {        // the windows that contain pixel (row, lx + j): origins (row .. + HALO, lx + j + PADX - HALO .. + HALO)
          const int o = (row + dy) * G::MW + lx + G::PADX - G::HALO;
          double va[G::NV], vb[G::NV], vc[G::NV];
#pragma unroll
          for (int j = 0; j < G::NV; ++j) va[j] = ma[o + j], vb[j] = mb[o + j], vc[j] = mc[o + j];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int dx = 0; dx < WIN; ++dx) sa[j] += va[j + dx], sb[j] += vb[j + dx], sc[j] += vc[j + dx];
          }
        }
        const int ctr = (row + G::HALO) * G::LS + G::PADX + lx;
        double d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = (double)sp[ctr + j] * sa[j] + (double)sx[ctr + j] * sb[j] + sc[j];
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
  }

  double v2[2] = {s_rho, s_hinge};
  __syncthreads();
  tmdiff::wg_sum<NT / 64, 2, 2>(v2, red);
  if (t == 0) {
    p.part[2 * (long)blockIdx.x] = v2[0];
    p.part[2 * (long)blockIdx.x + 1] = v2[1];
  }
}

struct LcorrFinalArgs {
  const double* part;   // [B * tiles][2]
  int B;
  long tiles;
  double per_image;     // windows of one image: C (H - win + 1)(W - win + 1)
  double weight;
  double* out64;        // [2] = loss, mean rho
  double* img_rho;      // null, or [B]: the mean rho of each image
  float* out32;         // weight * loss
};

// Image by image: lane t adds the image's workgroups t, t + 256, ... in order, then the workgroup sum: the order depends on the
// tile count alone.  The images' sums are then added in ascending order.
__global__ void __launch_bounds__(FIN_T) local_corr_finalize(LcorrFinalArgs p) {
  __shared__ double red[(FIN_T / 64) * 2];
  double tot_rho = 0.0, tot_hinge = 0.0;
  for (int b = 0; b < p.B; ++b) {
    const double* src = p.part + 2 * (long)b * p.tiles;
    double v[2] = {tmdiff::strided_sum(src, p.tiles, 2, threadIdx.x, FIN_T), tmdiff::strided_sum(src + 1, p.tiles, 2, threadIdx.x, FIN_T)};
    __syncthreads();                              // the lanes of image b - 1 have read red
    tmdiff::wg_sum<FIN_T / 64, 2, 2>(v, red);
    if (threadIdx.x == 0 && p.img_rho) p.img_rho[b] = v[0] / p.per_image;
    tot_rho += v[0];
    tot_hinge += v[1];
  }
  if (threadIdx.x != 0) return;
  const double nwin = p.per_image * p.B, loss = tot_hinge / nwin;
  p.out64[0] = loss;
  p.out64[1] = tot_rho / nwin;
  *p.out32 = (float)(p.weight * loss);
}

bool lcorr_ok(int B, int C, int H, int W, int win) {
  return B >= 1 && C >= 1 && C <= 16 && win >= 2 && win <= 8 && H >= win && W >= win && tmdiff::fits_int32((double)B * C * H * W);
}

size_t lcorr_bytes(int B, int H, int W) { return (size_t)B * tiles_of(H, W) * 2 * sizeof(double); }

}  // namespace

extern "C" {

int tmdiff_local_corr_loss_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t win) {
  return lcorr_ok(B, C, H, W, win);   // a predicate: it leaves the last-error string alone
}

size_t tmdiff_local_corr_loss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t win) {
  return lcorr_ok(B, C, H, W, win) ? lcorr_bytes(B, H, W) : 0;
}

int tmdiff_local_corr_loss(const float* x, const float* pan, float* g, const double* rho_max, int32_t win, double weight,
                           int32_t accumulate, double* out64, double* per_image, float* out32, void* workspace,
                           size_t workspace_bytes, int32_t B, int32_t C, int32_t H, int32_t W, tmdiff_stream_t stream) {
  if (!lcorr_ok(B, C, H, W, win))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "local_corr_loss: B=%d C=%d H=%d W=%d win=%d (B >= 1, 1 <= C <= 16, 2 <= win <= 8, "
                        "H, W >= win, fewer than 2^31 elements)", B, C, H, W, win);
  if (!(weight >= 0.0 && weight <= DBL_MAX))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "local_corr_loss: weight=%g (>= 0 and finite)", weight);
  TMDIFF_REQUIRE(x && pan && out64 && out32 && workspace, "local_corr_loss: null tensor");
  TMDIFF_REQUIRE(g || !accumulate, "local_corr_loss: accumulate needs a gradient tensor");
  TMDIFF_REQUIRE(((reinterpret_cast<uintptr_t>(rho_max) | reinterpret_cast<uintptr_t>(per_image)) & 7u) == 0,
                 "local_corr_loss: rho_max and per_image must be 8-byte aligned");
  if (const int rc = tmdiff::check_workspace("local_corr_loss", workspace, workspace_bytes, lcorr_bytes(B, H, W), ", as out64", out64))
    return rc;
  const hipStream_t st = tmdiff::as_stream(stream);
  const long tiles = tiles_of(H, W), blocks = (long)B * tiles;
  if (const int rc = tmdiff::check_grid(blocks, "local_corr_loss", TMDIFF_E_UNSUPPORTED)) return rc;
  const bool vec = W % 4 == 0 && tmdiff::aligned16(x) && tmdiff::aligned16(pan) && (!g || tmdiff::aligned16(g));
  const double per_img = (double)C * (H - win + 1) * (W - win + 1), nwin = per_img * B;
  const LcorrArgs a{x, pan, g, rho_max, C, H, W, (W + TW - 1) / TW, (int)tiles, vec, accumulate != 0, -weight / nwin,
                    static_cast<double*>(workspace)};
  switch (win) {
    case 2: local_corr_kernel<2><<<(unsigned)blocks, NT, 0, st>>>(a); break;
    case 3: local_corr_kernel<3><<<(unsigned)blocks, NT, 0, st>>>(a); break;
    case 4: local_corr_kernel<4><<<(unsigned)blocks, NT, 0, st>>>(a); break;
    case 5: local_corr_kernel<5><<<(unsigned)blocks, NT, 0, st>>>(a); break;
    case 6: local_corr_kernel<6><<<(unsigned)blocks, NT, 0, st>>>(a); break;
    case 7: local_corr_kernel<7><<<(unsigned)blocks, NT, 0, st>>>(a); break;
    default: local_corr_kernel<8><<<(unsigned)blocks, NT, 0, st>>>(a); break;
  }
  if (const int rc = tmdiff::check_launch("local_corr_loss")) return rc;
  const LcorrFinalArgs f{a.part, B, tiles, per_img, weight, out64, per_image, out32};
  local_corr_finalize<<<1, FIN_T, 0, st>>>(f);
  return tmdiff::check_launch("local_corr_loss (finalize)");
}

}  // extern "C"

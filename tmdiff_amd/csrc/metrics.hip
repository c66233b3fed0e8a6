// Pansharpening quality metrics on the device (gfx950): PSNR, SAM, SSIM, ERGAS, RMSE, CC, SCC, Q, Q4 of a prediction against a
// target, and D_lambda, D_s, QNR without a target -- the definitions of tmdiff_amd/metrics.py (reference core/metrics.py:56-284,
// :411-503), on fp32 [B, C, H, W] tensors whose batch and channel strides are arguments (rows and planes are dense).
//
//  metrics_pair_kernel   one workgroup per 16 x 64 tile of one image.  It walks the bands with the tile and a 3-pixel halo of both
//                        images in LDS, and forms per band 12 sums: a, b, a^2, b^2, ab, (a-b)^2 over the tile's pixels; the SSIM
//                        values of the 7 x 7 windows centred in the tile (window sums separably: rows first, through LDS); and
//                        the five moments of the two 3 x 3 Laplacians centred in the tile; and the least and greatest value of
//                        either image (a band is constant exactly when they agree).  The spectral sums of each pixel (dot,
//                        |a|^2, |b|^2) stay in registers across the band loop and become one angle per pixel after it; with four
//                        bands the pixel's eight values stay too and give the 4 x 4 cross products of Q4.
//  metrics_gram_kernel   channel sums and the upper triangle of sum x_i x_j over a list of up to 17 channels in two segments.
//  *_finalize_kernel     one workgroup per image: adds the workgroups' partial sums (stats.h strided_sum, wg_sum), evaluates the
//                        formulas.
//  metrics_q2n_kernel    Q2n (Q4 / Q8, metrics.q2n): one workgroup per block x block window of one image, both images' window in
//                        LDS as fp32 (mirrored at the bottom and the right while staging, zero bands up to a power of two).  Pass
//                        one: per band the mean and the centred sums of the ground truth and of the fused image about that mean.
//                        Pass two: the C x C matrix of centred cross products, each lane a T x T tile of band pairs over a slice
//                        of the pixels.  The normalised moments the definition asks for are affine in these, so no lane divides
//                        per pixel.  The workgroup then evaluates the hypercomplex product through the sign table and stores the
//                        block's value; metrics_q2n_finalize_kernel averages them per image.
//  metrics_dsblock_kernel  the spatial term of HQNR (metrics.d_s_block): one workgroup per block x block window of one image.
//                        The windows of pan and of the low-pass pan are staged once (mirrored like Q2n's), those of the fused
//                        and the interpolated MS image band by band; per band two passes over LDS, the means and then the
//                        centred sums, give Q(ps_c, pan) and Q(ms_c, pan_lp) of the window.
//                        metrics_dsblock_finalize_kernel averages the windows per band, forms D_s and, given the image's
//                        D_lambda, HQNR.
//
// Every sum is fp64 (products of two fp32 values are exact there): at sensor scale (mean 1000, sigma 5) a variance is a 4e4-th
// of the raw second moment, which fp32 sums would lose entirely.  No atomics: each workgroup adds through stats.h's workgroup sum
// and stores its partial sums with plain vector stores, and the finalize kernel adds them in index order, so a call is
// reproducible bit for bit.  Nothing is allocated, copied to the host or synchronised here: the caller lends the workspace and the
// launches go to its stream.
#include <algorithm>

#include "classical.h"

namespace {

constexpr int TH = 16, TW = 64, HALO = 3;            // tile owned by a workgroup; 256 lanes: lane (x, q) owns rows 4q .. 4q+3 of column x
constexpr int LH = TH + 2 * HALO, LW = TW + 2 * HALO;
constexpr int LS = 72;                               // LDS row stride of the staged tile (floats)
constexpr int NSUM = 12, NBAND = 16;                 // per band: 12 sums, then min a, max a, min b, max b
constexpr int RED = NBAND + 5;                       // columns of a wave's row of totals
constexpr int FIN_T = 1024, FIN_W = FIN_T / 64;      // finalize: 16 waves, each adds a fixed run of the tiles
constexpr int MAXC = 16, MAXG = 17;                  // bands of a pair; channels of a gram
constexpr int PAIR_K = 9, NOREF_K = 3;               // output columns
constexpr int GRAM_PIX = 256, GRAM_WG = 64;          // pixels per staged chunk; workgroups per image at most
constexpr int MAXENT = MAXG + MAXG * (MAXG + 1) / 2; // 170

__host__ __device__ inline int pair_np(int C) { return NBAND * C + 17; }   // + the angle sum + 16 cross products
inline int tiles_of(int H, int W) { return ((H + TH - 1) / TH) * ((W + TW - 1) / TW); }
inline int gram_wgs(long n) { return (int)std::min<long>((n + GRAM_PIX - 1) / GRAM_PIX, GRAM_WG); }
__host__ __device__ inline int gram_entries(int ch) { return ch + ch * (ch + 1) / 2; }

struct PairArgs {
  const float* a;   // x_true
  const float* b;   // x_pred
  long asB, asC, bsB, bsC;
  int C, H, W, tiles_x, tiles;
  double c1, c2;
  double* part;     // [B][tiles][pair_np(C)]
};

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

__global__ void __launch_bounds__(256) metrics_pair_kernel(PairArgs p) {
  __shared__ float sa[LH][LS], sb[LH][LS];
  __shared__ double hs[5][LH][TW];        // row sums over 7 columns of a, b, a^2, b^2, ab
  __shared__ double red[4][RED];          // per-wave sums (17 columns: the band's 12, or the angle + 16 cross products)

  const int t = threadIdx.x, x = t & 63, q = t >> 6;
  const int img = blockIdx.x / p.tiles, tile = blockIdx.x - img * p.tiles;
  const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
  const int y0 = ty * TH, x0 = tx * TW;
  const int H = p.H, W = p.W, C = p.C;
  const int gx = x0 + x;
  double* part = p.part + ((long)img * p.tiles + tile) * pair_np(C);

  double dot[4] = {0, 0, 0, 0}, na[4] = {0, 0, 0, 0}, nb[4] = {0, 0, 0, 0};
  float av[4][4], bv[4][4];               // [band][row]: kept for C == 4 only
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int r = 0; r < 4; ++r) av[k][r] = bv[k][r] = 0.f;

  for (int c = 0; c < C; ++c) {
    const float* pa = p.a + (long)img * p.asB + (long)c * p.asC;
    const float* pb = p.b + (long)img * p.bsB + (long)c * p.bsC;
    tmdiff::stage_halo_tile<float, LH, LW, LS, 256>(sa[0], sb[0], pa, pb, nullptr, y0 - HALO, x0 - HALO, H, W, false);
    __syncthreads();

    double s[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) s[k] = 0.0;
    float lo_a = INFINITY, hi_a = -INFINITY, lo_b = INFINITY, hi_b = -INFINITY;
    // point moments, the pixel's spectral sums, the Laplacians
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ly = q * 4 + r + HALO, lx = x + HALO, gy = y0 + q * 4 + r;
      if (gy < H && gx < W) {
        const float fa = sa[ly][lx], fb = sb[ly][lx];
        const double a = fa, b = fb, d = a - b;
        s[0] += a; s[1] += b; s[2] += a * a; s[3] += b * b; s[4] += a * b; s[5] += d * d;
        dot[r] += a * b; na[r] += a * a; nb[r] += b * b;
        lo_a = fminf(lo_a, fa); hi_a = fmaxf(hi_a, fa); lo_b = fminf(lo_b, fb); hi_b = fmaxf(hi_b, fb);
        if (C == 4) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (c == k) av[k][r] = fa, bv[k][r] = fb;
        }
        if (gy >= 1 && gy <= H - 2 && gx >= 1 && gx <= W - 2) {
          double ba = 0.0, bb = 0.0;
#pragma unroll
          for (int i = -1; i <= 1; ++i)
#pragma unroll
            for (int j = -1; j <= 1; ++j) ba += (double)sa[ly + i][lx + j], bb += (double)sb[ly + i][lx + j];
          const double la = 9.0 * a - ba, lb = 9.0 * b - bb;
          s[7] += la; s[8] += lb; s[9] += la * la; s[10] += lb * lb; s[11] += la * lb;
        }
      }
    }
    // 7-column sums of every staged row
    for (int i = t; i < LH * TW; i += 256) {
      const int ly = i >> 6, cx = i & 63;
      double h0 = 0, h1 = 0, h2 = 0, h3 = 0, h4 = 0;
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const double a = sa[ly][cx + j], b = sb[ly][cx + j];
        h0 += a; h1 += b; h2 += a * a; h3 += b * b; h4 += a * b;
      }
      hs[0][ly][cx] = h0; hs[1][ly][cx] = h1; hs[2][ly][cx] = h2; hs[3][ly][cx] = h3; hs[4][ly][cx] = h4;
    }
    __syncthreads();
    // 7-row sums of those -> the window moments of the four window centres this lane owns
    {
      double w[5][4];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        double v[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) v[j] = hs[k][q * 4 + j][x];
        const double mid = (v[3] + v[4]) + (v[5] + v[6]);
        w[k][0] = ((v[0] + v[1]) + v[2]) + mid;
        w[k][1] = ((v[1] + v[2]) + v[7]) + mid;
        w[k][2] = ((v[2] + v[7]) + v[8]) + mid;
        w[k][3] = ((v[7] + v[8]) + v[9]) + mid;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gy = y0 + q * 4 + r;
        if (gy >= HALO && gy <= H - 1 - HALO && gx >= HALO && gx <= W - 1 - HALO) {
          const double ux = w[0][r] / 49.0, uy = w[1][r] / 49.0;
          const double cn = 49.0 / 48.0;                                  // sample covariance
          const double vx = cn * (w[2][r] / 49.0 - ux * ux), vy = cn * (w[3][r] / 49.0 - uy * uy);
          const double vxy = cn * (w[4][r] / 49.0 - ux * uy);
          s[6] += ((2.0 * ux * uy + p.c1) * (2.0 * vxy + p.c2)) / ((ux * ux + uy * uy + p.c1) * (vx + vy + p.c2));
        }
      }
    }
    tmdiff::wg_sum_store<NSUM, RED>(s, red[0]);
    {
      const float m0 = wave_min(lo_a), m1 = wave_max(hi_a), m2 = wave_min(lo_b), m3 = wave_max(hi_b);
      if (x == 0) red[q][NSUM] = m0, red[q][NSUM + 1] = m1, red[q][NSUM + 2] = m2, red[q][NSUM + 3] = m3;
    }
    __syncthreads();
    if (t < NSUM) part[c * NBAND + t] = tmdiff::wg_sum_col<4, RED>(red[0], t);
    else if (t < NBAND) {
      const bool least = ((t - NSUM) & 1) == 0;   // a wave without a pixel of the image holds +inf / -inf
      const double u = least ? fmin(red[0][t], red[1][t]) : fmax(red[0][t], red[1][t]);
      const double v = least ? fmin(red[2][t], red[3][t]) : fmax(red[2][t], red[3][t]);
      part[c * NBAND + t] = least ? fmin(u, v) : fmax(u, v);
    }
  }

  // the spectral angle of each pixel: dot / |pred| / |true|, then acos; a non-finite angle (a zero spectrum, a ratio that rounds
  // above 1) counts as 0
  double e[17];
#pragma unroll
  for (int k = 0; k < 17; ++k) e[k] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gy = y0 + q * 4 + r;
    if (gy < H && gx < W) {
      const double ang = acos(dot[r] / sqrt(nb[r]) / sqrt(na[r]));
      e[0] += isfinite(ang) ? ang : 0.0;
      if (C == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) e[1 + i * 4 + j] += (double)av[i][r] * (double)bv[j][r];
      }
    }
  }
  __syncthreads();   // the last band's readers of `red` are done
  tmdiff::wg_sum_store<17, RED>(e, red[0]);
  __syncthreads();
  if (t < 17) part[C * NBAND + t] = tmdiff::wg_sum_col<4, RED>(red[0], t);
}

struct PairFinalArgs {
  const double* part;
  int C, H, W, tiles;
  double data_range, ratio;
  double* out;   // [B][PAIR_K]
};

// entry e of a tile's partial sums: 0 = a sum, 1 = a least value, 2 = a greatest value
__device__ __forceinline__ int entry_kind(int e, int C) {
  const int k = e % NBAND;
  return e < C * NBAND && k >= NSUM ? 1 + ((k - NSUM) & 1) : 0;
}
__device__ __forceinline__ double combine(int kind, double u, double v) { return kind == 0 ? u + v : kind == 1 ? fmin(u, v) : fmax(u, v); }

// Wave g adds tiles [g * run, (g + 1) * run) in index order, lane l the entries l, l + 64, ...; then the 16 runs are added in
// order: the order depends on the number of tiles alone.
__global__ void __launch_bounds__(FIN_T) metrics_pair_finalize_kernel(PairFinalArgs p) {
  __shared__ double runs[FIN_W][NBAND * MAXC + 17];
  __shared__ double tot[NBAND * MAXC + 17];
  const int np = pair_np(p.C), img = blockIdx.x, lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int run = (p.tiles + FIN_W - 1) / FIN_W, i0 = g * run, i1 = min(i0 + run, p.tiles);
  for (int e = lane; e < np; e += 64) {
    const int kind = entry_kind(e, p.C);
    const double* src = p.part + (long)img * p.tiles * np + e;
    double s = kind == 0 ? 0.0 : kind == 1 ? (double)INFINITY : -(double)INFINITY;
    for (int i = i0; i < i1; ++i) s = combine(kind, s, src[(long)i * np]);
    runs[g][e] = s;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < np; e += FIN_T) {
    const int kind = entry_kind(e, p.C);
    double s = runs[0][e];
    for (int k = 1; k < FIN_W; ++k) s = combine(kind, s, runs[k][e]);
    tot[e] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int C = p.C;
  const double n = (double)p.H * (double)p.W, nwin = (double)(p.H - 6) * (double)(p.W - 6);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double psnr = 0, ssim = 0, erg = 0, sq = 0, cc = 0, scc = 0, qq = 0;
  for (int c = 0; c < C; ++c) {
    const double* s = tot + c * NBAND;
    const double ma = s[0] / n, mb = s[1] / n, mse = s[5] / n;
    psnr += 10.0 * log10(p.data_range * p.data_range / mse);
    ssim += s[6] / nwin;
    erg += mse / (mb * mb);
    sq += s[5];
    // centred second moments.  A constant band (least value == greatest value) has variance and covariance exactly 0, which the
    // raw moments only give up to rounding (n v^2 is not exact for most v): they are set, so that such a band gives 0 / 0 = NaN
    // as the two-pass host evaluation does.  (Its Laplacian is exactly 0 at every pixel, so lc below needs no such care.)
    const bool const_a = s[12] == s[13], const_b = s[14] == s[15];
    const double va = const_a ? 0.0 : s[2] - s[0] * ma, vb = const_b ? 0.0 : s[3] - s[1] * mb;
    const double cov = (const_a || const_b) ? 0.0 : s[4] - s[0] * mb;
    cc += cov / sqrt(va) / sqrt(vb);
    const double d1 = va / (n - 1.0), d2 = vb / (n - 1.0);
    qq += 4.0 * (cov / (n - 1.0)) * ma * mb / (d1 + d2) / (ma * ma + mb * mb);
    const double nl = (double)(p.H - 2) * (double)(p.W - 2);
    const double la = s[9] - s[7] * (s[7] / nl), lb = s[10] - s[8] * (s[8] / nl);
    const double lc = s[11] - s[7] * (s[8] / nl);
    scc += lc / sqrt(la) / sqrt(lb);
  }
  double* o = p.out + (long)img * PAIR_K;
  o[0] = psnr / C;
  o[1] = tot[C * NBAND] / n * 180.0 / 3.14159265358979323846;
  o[2] = ssim / C;
  o[3] = 100.0 * p.ratio * sqrt(erg / C);
  o[4] = sqrt(sq / n);
  o[5] = cc / C;
  o[6] = scc / C;
  o[7] = qq / C;
  double q4 = nan;
  if (C == 4) {
    // the mean quaternion product of the centred prediction with the conjugate of the centred target (metrics._q4_from_moments)
    const double* X = tot + C * NBAND + 1;   // X[i * 4 + j] = sum a_i b_j
    double m1[4], m2[4], s1 = 0, s2 = 0, e1 = 0, e2 = 0, r[4][4];
    for (int i = 0; i < 4; ++i) {
      m2[i] = tot[i * NBAND] / n; m1[i] = tot[i * NBAND + 1] / n;
      s2 += tot[i * NBAND + 2] / n - m2[i] * m2[i]; s1 += tot[i * NBAND + 3] / n - m1[i] * m1[i];
      e1 += m1[i] * m1[i]; e2 += m2[i] * m2[i];
    }
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) r[i][j] = (X[j * 4 + i] / n - m1[i] * m2[j]) * (j == 0 ? 1.0 : -1.0);
    const double c0 = r[0][0] - r[1][1] - r[2][2] - r[3][3], c1 = r[0][1] + r[1][0] + r[2][3] - r[3][2];
    const double c2 = r[0][2] - r[1][3] + r[2][0] + r[3][1], c3 = r[0][3] + r[1][2] - r[2][1] + r[3][0];
    q4 = 4.0 * sqrt(e1 * e2 * (c0 * c0 + c1 * c1 + c2 * c2 + c3 * c3)) / (s1 + s2) / (e1 + e2);
  }
  o[8] = q4;
}

struct GramArgs {
  const float* x0;   // c0 channels
  const float* x1;   // c1 channels (may be 0)
  long s0B, s0C, s1B, s1C;
  int c0, c1, n, wgs;   // n = H * W pixels per image
  double* part;         // [B][wgs][gram_entries(c0 + c1)]: the channel sums, then the rows of the upper triangle
};

__global__ void __launch_bounds__(256) metrics_gram_kernel(GramArgs p) {
  __shared__ float xs[GRAM_PIX][MAXG];
  __shared__ double red[256];
  const int t = threadIdx.x, ch = p.c0 + p.c1, nent = gram_entries(ch), ng = 256 / nent;
  const int img = blockIdx.x / p.wgs, wg = blockIdx.x - img * p.wgs;
  const int e = t % nent, g = t / nent;
  int ei = e, ej = -1;                       // entry e: the sum of channel ei (ej < 0) or of x_ei x_ej
  if (e >= ch) {
    int k = e - ch;
    ei = 0;
    while (k >= ch - ei) k -= ch - ei, ++ei;
    ej = ei + k;
  }
  double acc = 0.0;
  const int chunks = (p.n + GRAM_PIX - 1) / GRAM_PIX;
  for (int chunk = wg; chunk < chunks; chunk += p.wgs) {
    const int px = chunk * GRAM_PIX + t, cnt = min(GRAM_PIX, p.n - chunk * GRAM_PIX);
    __syncthreads();
    for (int c = 0; c < ch; ++c) {
      const float* src = c < p.c0 ? p.x0 + (long)img * p.s0B + (long)c * p.s0C : p.x1 + (long)img * p.s1B + (long)(c - p.c0) * p.s1C;
      xs[t][c] = t < cnt ? src[px] : 0.f;
    }
    __syncthreads();
    if (g < ng)
      for (int i = g; i < cnt; i += ng) acc += ej < 0 ? (double)xs[i][ei] : (double)xs[i][ei] * (double)xs[i][ej];
  }
  red[t] = acc;
  __syncthreads();
  if (t < nent) {
    double s = 0.0;
    for (int k = 0; k < ng; ++k) s += red[k * nent + t];
    p.part[((long)img * p.wgs + wg) * nent + t] = s;
  }
}

struct NorefFinalArgs {
  const double* hi;   // gram partials of (ps, pan) over H x W
  const double* lo;   // ... of (l_ms, l_pan) over h x w
  int C, wgs_hi, wgs_lo;
  double n_hi, n_lo;
  double* out;        // [B][NOREF_K]
};

// QIndex of channels i < j from the totals: population moments, eps = 1e-8 in the denominator (core/metrics.py:442-461)
__device__ double q_pop(const double* tot, int ch, double n, int i, int j) {
  auto g = [&](int a, int b) { return tot[ch + a * ch - a * (a - 1) / 2 + (b - a)]; };
  const double ea = tot[i] / n, eb = tot[j] / n;
  const double va = g(i, i) / n - ea * ea, vb = g(j, j) / n - eb * eb, cab = g(i, j) / n - ea * eb;
  return 4.0 * cab * ea * eb / ((va + vb) * (ea * ea + eb * eb) + 1e-8);
}

__global__ void __launch_bounds__(256) metrics_noref_finalize_kernel(NorefFinalArgs p) {
  __shared__ double tot[2][MAXENT];
  const int ch = p.C + 1, nent = gram_entries(ch), img = blockIdx.x;
  for (int e = threadIdx.x; e < 2 * nent; e += 256) {
    const int which = e / nent, k = e - which * nent, wgs = which ? p.wgs_lo : p.wgs_hi;
    const double* src = (which ? p.lo : p.hi) + (long)img * wgs * nent + k;
    double s = 0.0;
    for (int i = 0; i < wgs; ++i) s += src[(long)i * nent];
    tot[which][k] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int L = p.C;
  double dl = 0.0, ds = 0.0;
  for (int i = 0; i < L; ++i) {
    for (int j = i + 1; j < L; ++j) dl += 2.0 * fabs(q_pop(tot[0], ch, p.n_hi, i, j) - q_pop(tot[1], ch, p.n_lo, i, j));
    ds += fabs(q_pop(tot[0], ch, p.n_hi, i, L) - q_pop(tot[1], ch, p.n_lo, i, L));
  }
  dl = dl / L / (double)(L - 1);   // one band: 0 / 0
  ds = ds / L;
  double* o = p.out + (long)img * NOREF_K;
  o[0] = dl; o[1] = ds; o[2] = (1.0 - dl) * (1.0 - ds);
}

// ---- Q2n --------------------------------------------------------------------------------------------------------------------
constexpr int Q2N_PAD = 4;   // floats after each staged band: the four band tiles a wave reads then fall on different LDS banks

struct Q2nArgs {
  const float* a;   // ground truth
  const float* b;   // fused
  long asB, asC, bsB, bsC;
  int C, Cp, H, W, block, shift, nx, nblk;   // Cp: C padded to a power of two; nblk = ny * nx
  unsigned long long neg[4];                 // bit i * 16 + j: e_i e_j = -e_(i xor j)
  double* vals;     // [B][nblk]
  double* map;      // [B][nblk] or null
};

__host__ __device__ inline int q2n_tile(int Cp) { return Cp < 4 ? Cp : 4; }   // a lane owns a T x T tile of band pairs

// Sum of N values per lane over groups of G consecutive lanes (G a power of two, 16 <= G <= 256, the same for the whole
// workgroup): every lane of a group gets the group's sum.  The order of stats.h over a group: the butterfly over the group's
// lanes of a wave (offsets from half the group's lanes down to 1: its own loop, the only one narrower than a wave), then the
// group's waves in order through red[4][16]; G = 256 is the workgroup sum.
template <int N>
__device__ __forceinline__ void group_sum(double (&v)[N], int G, double (*red)[16], int t) {
  const int gw = G < 64 ? G : 64;
#pragma unroll
  for (int k = 0; k < N; ++k)
    for (int m = gw >> 1; m >= 1; m >>= 1) v[k] += __shfl_xor(v[k], m, 64);
  if (G > 64) {
    const int wave = t >> 6, wpg = G >> 6, w0 = (wave / wpg) * wpg;
    __syncthreads();   // earlier readers of red are done
    if ((t & 63) == 0)
#pragma unroll
      for (int k = 0; k < N; ++k) red[wave][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = tmdiff::waves_in_order<16>(red[0], k, w0, wpg);
  }
}

template <int T>
__device__ __forceinline__ void q2n_gram(const float* sg, const float* sf, int bs, int n, int Cp, const double* mean, double (*gram)[16],
                                         double (*red)[16], int t) {
  const int tpr = Cp / T, tiles = tpr * tpr, slices = 256 / tiles;   // 16 / 64 / 256 / 256 / 256 slices for Cp = 16 / 8 / 4 / 2 / 1
  const int tile = t / slices, s = t - tile * slices, i0 = (tile / tpr) * T, j0 = (tile % tpr) * T;
  double mi[T], mj[T], acc[T * T];
#pragma unroll
  for (int u = 0; u < T; ++u) mi[u] = mean[i0 + u], mj[u] = mean[j0 + u];
#pragma unroll
  for (int u = 0; u < T * T; ++u) acc[u] = 0.0;
  for (int p = s; p < n; p += slices) {
    double dg[T], df[T];
#pragma unroll
    for (int u = 0; u < T; ++u) dg[u] = (double)sg[(i0 + u) * bs + p] - mi[u], df[u] = (double)sf[(j0 + u) * bs + p] - mj[u];
#pragma unroll
    for (int u = 0; u < T; ++u)
#pragma unroll
      for (int v = 0; v < T; ++v) acc[u * T + v] += dg[u] * df[v];
  }
  group_sum<T * T>(acc, slices, red, t);
  if (s == 0)
#pragma unroll
    for (int u = 0; u < T; ++u)
#pragma unroll
      for (int v = 0; v < T; ++v) gram[i0 + u][j0 + v] = acc[u * T + v];
}

__global__ void __launch_bounds__(256) metrics_q2n_kernel(Q2nArgs p) {
  extern __shared__ float q2n_lds[];         // [2][Cp][n + Q2N_PAD]: the window of a, then of b
  __shared__ double st[7][16];               // per band: mean a, divisor of x, divisor of y, sum dg, sum dg^2, sum df, sum df^2
  __shared__ double gram[16][16];            // sum over pixels of dg_i df_j
  __shared__ double red[4][16];
  __shared__ double qv[16];

  const int t = threadIdx.x, Cp = p.Cp, block = p.block, n = block * block, bs = n + Q2N_PAD;
  const int img = blockIdx.x / p.nblk, blk = blockIdx.x - img * p.nblk;
  const int by = blk / p.nx, bx = blk - by * p.nx, y0 = by * p.shift, x0 = bx * p.shift;
  float* sg = q2n_lds;
  float* sf = q2n_lds + Cp * bs;

  tmdiff::stage_mirrored<256, true, 2>({sg, sf}, {p.a + (long)img * p.asB, p.b + (long)img * p.bsB}, {p.asC, p.bsC}, p.C, Cp, bs, block,
                                       y0, x0, p.H, p.W);
  __syncthreads();

  // pass one: 256 / Cp lanes per band
  {
    const int G = 256 / Cp, c = t / G, l = t - c * G;
    double m[1] = {0.0};
    for (int px = l; px < n; px += G) m[0] += (double)sg[c * bs + px];
    group_sum<1>(m, G, red, t);
    const double mean = m[0] / (double)n;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int px = l; px < n; px += G) {
      const double dg = (double)sg[c * bs + px] - mean, df = (double)sf[c * bs + px] - mean;
      s[0] += dg; s[1] += dg * dg; s[2] += df; s[3] += df * df;
    }
    group_sum<4>(s, G, red, t);
    if (l == 0) {
      double sd = sqrt(s[1] / (double)(n - 1));
      if (sd == 0.0) sd = 0x1p-52;
      st[0][c] = mean; st[1][c] = sd; st[2][c] = mean == 0.0 ? 1.0 : sd;
      st[3][c] = s[0]; st[4][c] = s[1]; st[5][c] = s[2]; st[6][c] = s[3];
    }
  }
  __syncthreads();

  // pass two: the cross products
  if (Cp >= 4) q2n_gram<4>(sg, sf, bs, n, Cp, st[0], gram, red, t);
  else if (Cp == 2) q2n_gram<2>(sg, sf, bs, n, Cp, st[0], gram, red, t);
  else q2n_gram<1>(sg, sf, bs, n, Cp, st[0], gram, red, t);
  __syncthreads();

  // the block's value.  With u_i = sum dg_i / sx_i and w_j = sum df_j / sy_j:  sum x_i = u_i + n,  sum y_j = w_j + n,
  // sum x_i y_j = gram_ij / (sx_i sy_j) + u_i + w_j + n,  sum x_i^2 = sum dg_i^2 / sx_i^2 + 2 u_i + n, and y likewise.
  // No contraction here: t3 == 0 is an exact test that the host makes with separately rounded products.
  {
#pragma clang fp contract(off)
    const double nn = (double)n, k = nn / (nn - 1.0);
    double e1 = 0.0, e2 = 0.0, sxx = 0.0, syy = 0.0;
    for (int c = 0; c < Cp; ++c) {
      const double u = st[3][c] / st[1][c], w = st[5][c] / st[2][c];
      const double m1 = u / nn + 1.0, m2 = w / nn + 1.0;
      e1 += m1 * m1; e2 += m2 * m2;
      sxx += (st[4][c] / st[1][c] / st[1][c] + 2.0 * u + nn) / nn;
      syy += (st[6][c] / st[2][c] / st[2][c] + 2.0 * w + nn) / nn;
    }
    const double bias = 2.0 * sqrt(e1 * e2) / (e1 + e2);
    const double t3 = (k * sxx + k * syy) - k * (e1 + e2);
    if (t < Cp) {
      double q = 0.0;
      if (t3 == 0.0) {
        q = t == Cp - 1 ? bias : 0.0;
      } else {
        double ex = 0.0, mm = 0.0;   // component t of mean(x * y) and of m1 * m2: the pairs (i, i xor t)
        for (int i = 0; i < Cp; ++i) {
          const int j = i ^ t, bit = i * 16 + j;
          const double sgn = (((p.neg[bit >> 6] >> (bit & 63)) & 1ull) != 0) == (j != 0) ? 1.0 : -1.0;   // times y's conjugation
          const double u = st[3][i] / st[1][i], w = st[5][j] / st[2][j];
          const double xy = gram[i][j] / st[1][i] / st[2][j] + u + w + nn;
          ex += sgn * (xy / nn);
          mm += sgn * ((u / nn + 1.0) * (w / nn + 1.0));
        }
        q = (k * ex - k * mm) * bias * 2.0 / t3;
      }
      qv[t] = q * q;
    }
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int c = 0; c < Cp; ++c) s += qv[c];
    const double v = sqrt(s);
    p.vals[(long)img * p.nblk + blk] = v;
    if (p.map) p.map[(long)img * p.nblk + blk] = v;
  }
}

// Lane t adds the blocks t, t + 256, ... in order, then the workgroup sum: the order depends on the number of blocks alone.
__global__ void __launch_bounds__(256) metrics_q2n_finalize_kernel(const double* vals, int nblk, double* out) {
  __shared__ double red[4];
  const int t = threadIdx.x, img = blockIdx.x;
  const double s = tmdiff::block_sum_f64(tmdiff::strided_sum(vals + (long)img * nblk, nblk, 1, t, 256), red);
  if (t == 0) out[img] = s / (double)nblk;
}

// ---- block-wise D_s of HQNR ----------------------------------------------------------------------------------------------
struct DsArgs {
  const float* ps;    // fused image
  const float* ms;    // MS interpolated to the PAN grid
  const float* pan;   // one band
  const float* lp;    // low-pass PAN, one band
  long psB, psC, msB, msC, panB, lpB;
  int C, H, W, block, nx, nblk;
  double* vals;       // [B][C][2][nblk]: Q(ps_c, pan), then Q(ms_c, lp), per window
  double* map;        // the same layout, or null
};

// the workgroup sum of N values per lane, in every lane, behind a barrier: earlier readers of red are done
template <int N>
__device__ __forceinline__ void wg_sum(double (&v)[N], double (*red)[RED]) {
  __syncthreads();
  tmdiff::wg_sum<4, N, RED>(v, red[0]);
}

// metrics.q_index's formula from centred sums over n1 + 1 samples.  No contraction and the host's order of operations; a window
// constant in both images, or with both means zero, is 0 / 0 = NaN as on the host.
__device__ __forceinline__ double uqi_of(double saa, double sbb, double sab, double ma, double mb, double n1) {
#pragma clang fp contract(off)
  const double d1 = saa / n1, d2 = sbb / n1, cov = sab / n1;
  return 4.0 * cov * ma * mb / (d1 + d2) / (ma * ma + mb * mb);
}

__global__ void __launch_bounds__(256) metrics_dsblock_kernel(DsArgs p) {
  __shared__ float win[4][32 * 32];       // the window of ps_c, ms_c, pan, lp
  __shared__ double red[4][RED];

  const int t = threadIdx.x;
  const int block = p.block, n = block * block;
  const int img = blockIdx.x / p.nblk, blk = blockIdx.x - img * p.nblk;
  const int by = blk / p.nx, bx = blk - by * p.nx, y0 = by * block, x0 = bx * block;
  const double nn = (double)n, n1 = nn - 1.0;

  auto stage = [&](const float* src, float* dst) {
    tmdiff::stage_mirrored<256, false, 1>({dst}, {src}, {0}, 1, 1, 0, block, y0, x0, p.H, p.W);
  };
  stage(p.pan + (long)img * p.panB, win[2]);
  stage(p.lp + (long)img * p.lpB, win[3]);
  __syncthreads();

  // the two PAN windows serve every band: their means and centred squares once
  double mp[2] = {0.0, 0.0};
  for (int px = t; px < n; px += 256) mp[0] += (double)win[2][px], mp[1] += (double)win[3][px];
  wg_sum<2>(mp, red);
  mp[0] /= nn; mp[1] /= nn;
  double sp[2] = {0.0, 0.0};
  for (int px = t; px < n; px += 256) {
    const double dp = (double)win[2][px] - mp[0], dq = (double)win[3][px] - mp[1];
    sp[0] += dp * dp; sp[1] += dq * dq;
  }
  wg_sum<2>(sp, red);

  for (int c = 0; c < p.C; ++c) {
    __syncthreads();   // the last band's readers of win are done
    stage(p.ps + (long)img * p.psB + (long)c * p.psC, win[0]);
    stage(p.ms + (long)img * p.msB + (long)c * p.msC, win[1]);
    __syncthreads();
    double m[2] = {0.0, 0.0};
    for (int px = t; px < n; px += 256) m[0] += (double)win[0][px], m[1] += (double)win[1][px];
    wg_sum<2>(m, red);
    m[0] /= nn; m[1] /= nn;
    double s[4] = {0.0, 0.0, 0.0, 0.0};   // centred: a raw second moment at sensor scale would lose the variance
    for (int px = t; px < n; px += 256) {
      const double da = (double)win[0][px] - m[0], db = (double)win[1][px] - m[1];
      const double dp = (double)win[2][px] - mp[0], dq = (double)win[3][px] - mp[1];
      s[0] += da * da; s[1] += da * dp; s[2] += db * db; s[3] += db * dq;
    }
    wg_sum<4>(s, red);
    if (t == 0) {
      const double qh = uqi_of(s[0], sp[0], s[1], m[0], mp[0], n1), ql = uqi_of(s[2], sp[1], s[3], m[1], mp[1], n1);
      const long at = (((long)img * p.C + c) * 2) * p.nblk + blk;
      p.vals[at] = qh; p.vals[at + p.nblk] = ql;
      if (p.map) p.map[at] = qh, p.map[at + p.nblk] = ql;
    }
  }
}

struct DsFinalArgs {
  const double* vals;   // [B][C][2][nblk]
  int C, nblk;
  double q, alpha, beta;
  const double* dl;     // [B] D_lambda of each image, or null
  double* out;          // [B][2]: D_s, HQNR (left alone without dl)
};

__device__ __forceinline__ double pow_exact1(double x, double e) { return e == 1.0 ? x : e == 2.0 ? x * x : pow(x, e); }

// Per (band, high / low) lane t adds the windows t, t + 256, ... in order, then the workgroup sum: the order depends on the number
// of windows alone.
__global__ void __launch_bounds__(256) metrics_dsblock_finalize_kernel(DsFinalArgs p) {
  __shared__ double red[4][2 * MAXC];
  const int t = threadIdx.x, img = blockIdx.x;
  for (int k = 0; k < 2 * p.C; ++k) {
    const double s[1] = {tmdiff::strided_sum(p.vals + ((long)img * 2 * p.C + k) * p.nblk, p.nblk, 1, t, 256)};
    tmdiff::wg_sum_store<1, 2 * MAXC>(s, red[0] + k);
  }
  __syncthreads();
  if (t != 0) return;
  {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int c = 0; c < p.C; ++c) {
      const double qh = tmdiff::wg_sum_col<4, 2 * MAXC>(red[0], 2 * c) / (double)p.nblk;
      const double ql = tmdiff::wg_sum_col<4, 2 * MAXC>(red[0], 2 * c + 1) / (double)p.nblk;
      acc += pow_exact1(fabs(qh - ql), p.q);
    }
    acc /= (double)p.C;
    const double ds = p.q == 1.0 ? acc : p.q == 2.0 ? sqrt(acc) : pow(acc, 1.0 / p.q);
    p.out[(long)img * 2] = ds;
    if (p.dl) p.out[(long)img * 2 + 1] = pow_exact1(1.0 - p.dl[img], p.alpha) * pow_exact1(1.0 - ds, p.beta);
  }
}

// Cayley-Dickson product of two n-vectors (n a power of two; metrics.cd_mul): with p = (a, b), r = (c, d),
// p r = (a c - d conj(b), conj(a) d + c b)
void cd_mul(const double* p, const double* r, double* out, int n) {
  if (n == 1) { out[0] = p[0] * r[0]; return; }
  const int h = n / 2;
  double cb[8], ca[8], u[8], v[8];
  for (int i = 0; i < h; ++i) cb[i] = i ? -p[h + i] : p[h + i], ca[i] = i ? -p[i] : p[i];
  cd_mul(p, r, u, h); cd_mul(r + h, cb, v, h);
  for (int i = 0; i < h; ++i) out[i] = u[i] - v[i];
  cd_mul(ca, r + h, u, h); cd_mul(r, p + h, v, h);
  for (int i = 0; i < h; ++i) out[h + i] = u[i] + v[i];
}

// the signs of e_i e_j = +-e_(i xor j) for 16 components (the tables of 1, 2, 4 and 8 components are its leading blocks)
void q2n_signs(unsigned long long (&neg)[4]) {
  neg[0] = neg[1] = neg[2] = neg[3] = 0;
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < 16; ++j) {
      double ei[16] = {0}, ej[16] = {0}, o[16];
      ei[i] = ej[j] = 1.0;
      cd_mul(ei, ej, o, 16);
      if (o[i ^ j] < 0.0) neg[(i * 16 + j) >> 6] |= 1ull << ((i * 16 + j) & 63);
    }
}

int q2n_bands(int C) {
  int cp = 1;
  while (cp < C) cp *= 2;
  return cp;
}

struct Q2nGrid { int ny, nx; };
bool q2n_ok(int B, int C, int H, int W, int block, int shift, Q2nGrid* g = nullptr) {
  if (!(B >= 0 && C >= 1 && C <= MAXC && H >= 1 && W >= 1 && tmdiff::fits_int32((double)B * C * H * W))) return false;
  if (!(block == 8 || block == 16 || block == 32) || shift < 1 || shift > block) return false;
  const long ny = ((long)H + shift - 1) / shift, nx = ((long)W + shift - 1) / shift;
  if ((ny - 1) * shift + block - H > H || (nx - 1) * shift + block - W > W) return false;   // the mirror stays inside the image
  if (!tmdiff::fits_int32((double)B * ny * nx)) return false;
  if (g) g->ny = (int)ny, g->nx = (int)nx;
  return true;
}
size_t q2n_lds_bytes(int Cp, int block) { return (size_t)2 * Cp * (block * block + Q2N_PAD) * sizeof(float); }

bool extents_ok(int B, int C, int H, int W) {
  return B >= 0 && C >= 1 && C <= MAXC && H >= 7 && W >= 7 && tmdiff::fits_int32((double)B * C * H * W);
}

size_t pair_bytes(int B, int C, int H, int W) { return (size_t)B * tiles_of(H, W) * pair_np(C) * sizeof(double); }
size_t noref_bytes(int B, int C) { return (size_t)B * 2 * GRAM_WG * gram_entries(C + 1) * sizeof(double); }

}  // namespace

extern "C" {

int tmdiff_metrics_supported(int32_t B, int32_t C, int32_t H, int32_t W) {
  return extents_ok(B, C, H, W);   // a predicate: it leaves the last-error string alone
}

size_t tmdiff_metrics_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  if (!extents_ok(B, C, H, W)) return 0;
  return std::max(pair_bytes(B, C, H, W), noref_bytes(B, C));
}

int tmdiff_metrics_pair(const float* x_true, int64_t true_stride_b, int64_t true_stride_c, const float* x_pred, int64_t pred_stride_b,
                        int64_t pred_stride_c, int32_t B, int32_t C, int32_t H, int32_t W, double data_range, double ratio, double* out,
                        void* workspace, size_t workspace_bytes, tmdiff_stream_t stream) {
  if (!extents_ok(B, C, H, W))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "metrics_pair: B=%d C=%d H=%d W=%d (1 <= C <= 16, H, W >= 7, fewer than 2^31 elements)", B, C,
                        H, W);
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(x_true && x_pred && out && workspace, "metrics_pair: null tensor");
  TMDIFF_REQUIRE(true_stride_b >= 0 && true_stride_c >= (int64_t)H * W && pred_stride_b >= 0 && pred_stride_c >= (int64_t)H * W,
                 "metrics_pair: channel strides below a plane of %d x %d", H, W);
  if (const int rc = tmdiff::check_workspace("metrics_pair", workspace, workspace_bytes, pair_bytes(B, C, H, W))) return rc;
  const hipStream_t st = tmdiff::as_stream(stream);
  const int tiles_x = (W + TW - 1) / TW, tiles = tiles_of(H, W);
  const long blocks = (long)B * tiles;
  if (const int rc = tmdiff::check_grid(blocks, "metrics_pair", TMDIFF_E_UNSUPPORTED)) return rc;
  const PairArgs a{x_true, x_pred, true_stride_b, true_stride_c, pred_stride_b, pred_stride_c, C, H, W, tiles_x, tiles,
                   (0.01 * data_range) * (0.01 * data_range), (0.03 * data_range) * (0.03 * data_range), static_cast<double*>(workspace)};
  metrics_pair_kernel<<<(unsigned)blocks, 256, 0, st>>>(a);
  if (const int rc = tmdiff::check_launch("metrics_pair")) return rc;
  const PairFinalArgs f{a.part, C, H, W, tiles, data_range, ratio, out};
  metrics_pair_finalize_kernel<<<B, FIN_T, 0, st>>>(f);
  return tmdiff::check_launch("metrics_pair (finalize)");
}

int tmdiff_metrics_noref(const float* l_ms, int64_t l_ms_stride_b, int64_t l_ms_stride_c, const float* pan, int64_t pan_stride_b,
                         const float* l_pan, int64_t l_pan_stride_b, const float* ps, int64_t ps_stride_b, int64_t ps_stride_c, int32_t B,
                         int32_t C, int32_t H, int32_t W, int32_t h, int32_t w, double* out, void* workspace, size_t workspace_bytes,
                         tmdiff_stream_t stream) {
  if (!extents_ok(B, C, H, W) || h < 1 || w < 1 || !tmdiff::fits_int32((double)B * C * h * w))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "metrics_noref: B=%d C=%d H=%d W=%d h=%d w=%d (1 <= C <= 16, H, W >= 7, h, w >= 1, fewer than "
                        "2^31 elements)", B, C, H, W, h, w);
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(l_ms && pan && l_pan && ps && out && workspace, "metrics_noref: null tensor");
  TMDIFF_REQUIRE(ps_stride_b >= 0 && pan_stride_b >= 0 && l_ms_stride_b >= 0 && l_pan_stride_b >= 0 && ps_stride_c >= (int64_t)H * W &&
                     l_ms_stride_c >= (int64_t)h * w, "metrics_noref: channel strides below a plane");
  if (const int rc = tmdiff::check_workspace("metrics_noref", workspace, workspace_bytes, noref_bytes(B, C))) return rc;
  const hipStream_t st = tmdiff::as_stream(stream);
  const int nent = gram_entries(C + 1);
  double* hi = static_cast<double*>(workspace);
  const GramArgs gh{ps, pan, ps_stride_b, ps_stride_c, pan_stride_b, 0, C, 1, H * W, gram_wgs((long)H * W), hi};
  double* lo = hi + (size_t)B * gh.wgs * nent;
  const GramArgs gl{l_ms, l_pan, l_ms_stride_b, l_ms_stride_c, l_pan_stride_b, 0, C, 1, h * w, gram_wgs((long)h * w), lo};
  metrics_gram_kernel<<<(unsigned)(B * gh.wgs), 256, 0, st>>>(gh);
  if (const int rc = tmdiff::check_launch("metrics_noref (gram of ps, pan)")) return rc;
  metrics_gram_kernel<<<(unsigned)(B * gl.wgs), 256, 0, st>>>(gl);
  if (const int rc = tmdiff::check_launch("metrics_noref (gram of l_ms, l_pan)")) return rc;
  const NorefFinalArgs f{hi, lo, C, gh.wgs, gl.wgs, (double)H * W, (double)h * w, out};
  metrics_noref_finalize_kernel<<<B, 256, 0, st>>>(f);
  return tmdiff::check_launch("metrics_noref (finalize)");
}

int tmdiff_metrics_q2n_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t block, int32_t shift) {
  return q2n_ok(B, C, H, W, block, shift);
}

size_t tmdiff_metrics_q2n_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t block, int32_t shift) {
  Q2nGrid g;
  if (!q2n_ok(B, C, H, W, block, shift, &g)) return 0;
  return (size_t)B * g.ny * g.nx * sizeof(double);
}

int tmdiff_metrics_q2n(const float* x_true, int64_t true_stride_b, int64_t true_stride_c, const float* x_pred, int64_t pred_stride_b,
                       int64_t pred_stride_c, int32_t B, int32_t C, int32_t H, int32_t W, int32_t block, int32_t shift, double* out,
                       double* map_out, void* workspace, size_t workspace_bytes, tmdiff_stream_t stream) {
  Q2nGrid g;
  if (!q2n_ok(B, C, H, W, block, shift, &g))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "metrics_q2n: B=%d C=%d H=%d W=%d block=%d shift=%d (1 <= C <= 16, block 8, 16 or 32, 1 <= "
                        "shift <= block, mirror padding no longer than the axis, fewer than 2^31 elements)", B, C, H, W, block, shift);
  if (B == 0) return TMDIFF_OK;
  const size_t need = (size_t)B * g.ny * g.nx * sizeof(double);
  TMDIFF_REQUIRE(x_true && x_pred && out && workspace, "metrics_q2n: null tensor");
  TMDIFF_REQUIRE(true_stride_b >= 0 && true_stride_c >= (int64_t)H * W && pred_stride_b >= 0 && pred_stride_c >= (int64_t)H * W,
                 "metrics_q2n: channel strides below a plane of %d x %d", H, W);
  if (const int rc = tmdiff::check_workspace("metrics_q2n", workspace, workspace_bytes, need)) return rc;
  const hipStream_t st = tmdiff::as_stream(stream);
  const int Cp = q2n_bands(C);
  const size_t lds = q2n_lds_bytes(Cp, block);
  if (lds > 48 * 1024) {
    // more dynamic LDS than a launch gets by default: raise the kernel's limit once per device (131,584 bytes at the most)
    static size_t raised[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return tmdiff::fail(TMDIFF_E_LAUNCH, "metrics_q2n: no current device");
    if (raised[dev] < lds) {
      const size_t most = q2n_lds_bytes(MAXC, 32);
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(metrics_q2n_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
      if (e != hipSuccess) return tmdiff::fail(TMDIFF_E_LAUNCH, "metrics_q2n: %zu bytes of LDS: %s", most, hipGetErrorString(e));
      raised[dev] = most;
    }
  }
  Q2nArgs a{x_true, x_pred, true_stride_b, true_stride_c, pred_stride_b, pred_stride_c, C, Cp, H, W, block, shift, g.nx, g.ny * g.nx,
            {0, 0, 0, 0}, static_cast<double*>(workspace), map_out};
  static unsigned long long signs[4];
  static const bool signs_made = (q2n_signs(signs), true);
  (void)signs_made;
  for (int i = 0; i < 4; ++i) a.neg[i] = signs[i];
  metrics_q2n_kernel<<<(unsigned)((long)B * a.nblk), 256, lds, st>>>(a);
  if (const int rc = tmdiff::check_launch("metrics_q2n")) return rc;
  metrics_q2n_finalize_kernel<<<B, 256, 0, st>>>(a.vals, a.nblk, out);
  return tmdiff::check_launch("metrics_q2n (finalize)");
}

int tmdiff_metrics_dsblock_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t block) {
  return q2n_ok(B, C, H, W, block, block);
}

size_t tmdiff_metrics_dsblock_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t block) {
  Q2nGrid g;
  if (!q2n_ok(B, C, H, W, block, block, &g)) return 0;
  return (size_t)B * C * 2 * g.ny * g.nx * sizeof(double);
}

int tmdiff_metrics_dsblock(const float* ps, int64_t ps_stride_b, int64_t ps_stride_c, const float* ms_exp, int64_t ms_stride_b,
                           int64_t ms_stride_c, const float* pan, int64_t pan_stride_b, const float* pan_lp, int64_t pan_lp_stride_b,
                           int32_t B, int32_t C, int32_t H, int32_t W, int32_t block, double q, const double* d_lambda, double alpha,
                           double beta, double* out, double* maps_out, void* workspace, size_t workspace_bytes,
                           tmdiff_stream_t stream) {
  Q2nGrid g;
  if (!q2n_ok(B, C, H, W, block, block, &g) || !tmdiff::fits_int32((double)B * C * 2 * g.ny * g.nx))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "metrics_dsblock: B=%d C=%d H=%d W=%d block=%d (1 <= C <= 16, block 8, 16 or 32, mirror "
                        "padding no longer than the axis, fewer than 2^31 elements)", B, C, H, W, block);
  if (!(q > 0.0 && q <= 1e6) || !(alpha == alpha) || !(beta == beta))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "metrics_dsblock: q=%g alpha=%g beta=%g (q > 0, exponents not NaN)", q, alpha, beta);
  if (B == 0) return TMDIFF_OK;
  const size_t need = (size_t)B * C * 2 * g.ny * g.nx * sizeof(double);
  TMDIFF_REQUIRE(ps && ms_exp && pan && pan_lp && out && workspace, "metrics_dsblock: null tensor");
  TMDIFF_REQUIRE(ps_stride_b >= 0 && ps_stride_c >= (int64_t)H * W && ms_stride_b >= 0 && ms_stride_c >= (int64_t)H * W &&
                     pan_stride_b >= 0 && pan_lp_stride_b >= 0, "metrics_dsblock: channel strides below a plane of %d x %d", H, W);
  if (const int rc = tmdiff::check_workspace("metrics_dsblock", workspace, workspace_bytes, need)) return rc;
  const hipStream_t st = tmdiff::as_stream(stream);
  const DsArgs a{ps, ms_exp, pan, pan_lp, ps_stride_b, ps_stride_c, ms_stride_b, ms_stride_c, pan_stride_b, pan_lp_stride_b,
                 C, H, W, block, g.nx, g.ny * g.nx, static_cast<double*>(workspace), maps_out};
  metrics_dsblock_kernel<<<(unsigned)((long)B * a.nblk), 256, 0, st>>>(a);
  if (const int rc = tmdiff::check_launch("metrics_dsblock")) return rc;
  const DsFinalArgs f{a.vals, C, a.nblk, q, alpha, beta, d_lambda, out};
  metrics_dsblock_finalize_kernel<<<B, 256, 0, st>>>(f);
  return tmdiff::check_launch("metrics_dsblock (finalize)");
}

}  // extern "C"

// ---- The injection statistics of MTF-GLP (metrics.glp_moments): per band the population means, variances and the covariance of
// M = ms_exp and L = pan_lp, and the mean and variance of P = pan, as device values for glp_inject_kernel (fusion.hip).
//
//  glp_moments_kernel    one workgroup per chunk of 4096 consecutive pixels of one image; lane t owns the four pixels from
//                        chunk + 4 (256 k + t) on, k = 0 .. 3 (load_quad_minus_pilot, classical.h), and adds them in that order
//                        (k, then the pixel).  It reads P once, forms its two sums, then walks the
//                        bands with five sums each.  Seven partial sums per band and chunk go to the workspace.
//  glp_moments_finalize_kernel  one workgroup per (band, image): lane t adds chunks t, t + 256, ... (strided_sum), the
//                        workgroup adds the lanes (wg_sum), lane 0 forms the moments.
//
// CONDITIONING: the second moments are taken about a PILOT, not about zero and not about the mean: every value has the first
// pixel of its own plane subtracted in fp64 right after the load (exact for fp32 data of one binade range), d = v - v[0], and
// the sums are of d and of products of two d's.  mean = v[0] + S_d / n, var = S_dd / n - (S_d / n)^2: the subtraction that
// remains cancels at most (range / sigma)^2 of fp64's 2^53, where raw squares would cancel (mean / sigma)^2.  One pass over
// the images, no second pass for the means.  A constant plane has d == 0 everywhere and a variance of exactly 0.
// The finished sums are kept as well, ahead of the partial sums in the workspace: [B, C, 7] doubles in the order
// S_dm, S_dl, S_dp, S_dm.dm, S_dl.dl, S_dm.dl, S_dp.dp.  Summation order: stats.h, and nothing else; no atomics.
namespace {

constexpr int GLP_QUADS = 4, GLP_PIX = 256 * 4 * GLP_QUADS;   // pixels of a workgroup's chunk
constexpr int GLP_K = 7;

inline int glp_chunks(long n) { return (int)((n + GLP_PIX - 1) / GLP_PIX); }
inline size_t glp_bytes(int B, int C, int H, int W) {
  return ((size_t)B * C * GLP_K + (size_t)B * glp_chunks((long)H * W) * (5 * C + 2)) * sizeof(double);
}

struct GlpArgs {
  const float* m;   // ms_exp [B, C, n]
  const float* l;   // pan_lp [B, C, n]
  const float* p;   // pan    [B, n]
  int B, C, n, chunks, vec;
  double* sums;     // [B, C, 7]
  double* part;     // [B, chunks, 5 C + 2]
  double* out;      // [B, C, 7]
};

__global__ void __launch_bounds__(256) glp_moments_kernel(GlpArgs a) {
  __shared__ double red[4 * 5];
  const int chunk = blockIdx.x;
  const long px0 = (long)chunk * GLP_PIX + 4 * threadIdx.x;
  const int ld = 5 * a.C + 2;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    double* dst = a.part + ((long)b * a.chunks + chunk) * ld;
    {
      const float* pp = a.p + (long)b * a.n;
      const float pilot = pp[0];
      double v[2] = {0.0, 0.0};
#pragma unroll
      for (int k = 0; k < GLP_QUADS; ++k) {
        double d[4];
        tmdiff::load_quad_minus_pilot(pp, true, pilot, 0.f, px0 + k * 1024, a.n, a.vec, d);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[0] += d[e], v[1] += d[e] * d[e];
      }
      __syncthreads();                                            // the image before may still read red
      tmdiff::wg_sum<4, 2, 2>(v, red);
      if (threadIdx.x == 0) dst[5 * a.C] = v[0], dst[5 * a.C + 1] = v[1];
    }
    for (int c = 0; c < a.C; ++c) {
      const float* mp = a.m + ((long)b * a.C + c) * a.n;
      const float* lp = a.l + ((long)b * a.C + c) * a.n;
      const float pm = mp[0], pl = lp[0];
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < GLP_QUADS; ++k) {
        double dm[4], dl[4];
        tmdiff::load_quad_minus_pilot(mp, true, pm, 0.f, px0 + k * 1024, a.n, a.vec, dm);
        tmdiff::load_quad_minus_pilot(lp, true, pl, 0.f, px0 + k * 1024, a.n, a.vec, dl);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          v[0] += dm[e], v[1] += dl[e], v[2] += dm[e] * dm[e], v[3] += dl[e] * dl[e], v[4] += dm[e] * dl[e];
      }
      __syncthreads();                                            // the band before may still read red
      tmdiff::wg_sum<4, 5, 5>(v, red);
      if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) dst[5 * c + k] = v[k];
    }
  }
}

__global__ void __launch_bounds__(256) glp_moments_finalize_kernel(GlpArgs a) {
  __shared__ double red[4 * GLP_K];
  const int c = blockIdx.x, ld = 5 * a.C + 2;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    const double* src = a.part + (long)b * a.chunks * ld;
    double v[GLP_K];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = tmdiff::strided_sum(src + 5 * c + k, a.chunks, ld, threadIdx.x, 256);
    v[5] = tmdiff::strided_sum(src + 5 * a.C, a.chunks, ld, threadIdx.x, 256);
    v[6] = tmdiff::strided_sum(src + 5 * a.C + 1, a.chunks, ld, threadIdx.x, 256);
    __syncthreads();
    tmdiff::wg_sum<4, GLP_K, GLP_K>(v, red);
    if (threadIdx.x == 0) {
      const long bc = (long)b * a.C + c;
      const double n = (double)a.n, pm = a.m[bc * a.n], pl = a.l[bc * a.n], pp = a.p[(long)b * a.n];
      const double em = v[0] / n, el = v[1] / n, ep = v[5] / n;
      double* s = a.sums + bc * GLP_K;
      s[0] = v[0], s[1] = v[1], s[2] = v[5], s[3] = v[2], s[4] = v[3], s[5] = v[4], s[6] = v[6];
      double* o = a.out + bc * GLP_K;               // metrics.GLP_MOMENT_FIELDS
      o[0] = pm + em, o[1] = pl + el, o[2] = pp + ep;
      o[3] = v[2] / n - em * em, o[4] = v[3] / n - el * el, o[5] = v[4] / n - em * el, o[6] = v[6] / n - ep * ep;
    }
  }
}

}  // namespace

extern "C" {

size_t tmdiff_glp_moments_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  return tmdiff::planes_ok(B, C, MAXC, H, W) ? glp_bytes(B, C, H, W) : 0;
}

int tmdiff_glp_moments(const float* ms_exp, const float* pan, const float* pan_lp, int32_t B, int32_t C, int32_t H, int32_t W,
                       double* out, void* workspace, size_t workspace_bytes, tmdiff_stream_t stream) {
  if (!tmdiff::planes_ok(B, C, MAXC, H, W))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "glp_moments: B=%d C=%d H=%d W=%d (B >= 0, 1 <= C <= 16, H, W >= 1, fewer than 2^31 "
                        "elements)", B, C, H, W);
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(ms_exp && pan && pan_lp && out && workspace, "glp_moments: null tensor");
  if (const int rc = tmdiff::check_workspace("glp_moments", workspace, workspace_bytes, glp_bytes(B, C, H, W))) return rc;
  const hipStream_t st = tmdiff::as_stream(stream);
  const int n = H * W, chunks = glp_chunks(n);
  double* ws = static_cast<double*>(workspace);
  const int vec = n % 4 == 0 && tmdiff::aligned16(ms_exp) && tmdiff::aligned16(pan) && tmdiff::aligned16(pan_lp);
  const GlpArgs a{ms_exp, pan_lp, pan, B, C, n, chunks, vec, ws, ws + (size_t)B * C * GLP_K, out};
  glp_moments_kernel<<<dim3((unsigned)chunks, (unsigned)std::min(B, 65535)), 256, 0, st>>>(a);
  if (const int rc = tmdiff::check_launch("glp_moments")) return rc;
  glp_moments_finalize_kernel<<<dim3((unsigned)C, (unsigned)std::min(B, 65535)), 256, 0, st>>>(a);
  return tmdiff::check_launch("glp_moments (finalize)");
}

}  // extern "C"

// The composite finetune loss with its gradient in one pass (gfx950; host definition: tmdiff_amd/losses.py):
//
//   L = base(xh, x0) + w_sam * SAM(x0 + ms, xh + ms) + w_lap * LAP(xh - x0)          fp32 [B, C, H, W] tensors
//
//  base  mean over B C H W of rho(xh - x0): |d| (l1), d^2 (l2), or smooth l1 with beta = 1.
//  SAM   mean over the B H W pixels of the angle between the band vectors u = x0 + ms and v = xh + ms, as
//        atan2(|cross|, dot) with |cross|^2 = |u|^2 |v|^2 - dot^2 (Lagrange's identity: exactly 0 for parallel integer
//        vectors).  d angle / d v = -(u - (dot / |v|^2) v) / |cross|, a vector of norm 1 / |v|.  A pixel with |u| = 0,
//        |v| = 0 or |cross|^2 <= 0 contributes its angle (0, or pi for antiparallel vectors) and a zero gradient; with one band
//        every pixel does.
//  LAP   mean over the B C (H - 2)(W - 2) interior pixels of |Lap d|, Lap = the 3 x 3 kernel (1 1 1; 1 -8 1; 1 1 1); its
//        gradient is Lap^T applied to sign(Lap d), sign(0) = 0, taken as 0 outside the interior.
//
//  loss_kernel            one workgroup of 128 lanes per 16 x 32 tile of one image; a lane owns four neighbouring pixels of a
//                         row.  A first walk over the bands forms each pixel's dot, |u|^2, |v|^2 and from them the angle and
//                         the two coefficients of its gradient (w_sam = 0: skipped).  A second walk stages the tile of x0 and
//                         xh with a halo of 2 in LDS, writes sign(Lap d) of the tile and a halo of 1 into LDS (w_lap = 0: no
//                         LDS at all, the lanes read their own pixels), and stores g = dL/dxh for the band: weighted, divided
//                         by the counts, rounded to fp32 once.  16-byte accesses when W % 4 == 0 and the tensors are 16-byte
//                         aligned (the staged tile has a halo of 4 columns, so that a float4 lies inside the image or outside
//                         it), scalar ones otherwise.  g == NULL: values only.
//  loss_finalize_kernel   adds the workgroups' three partial sums (in index order, then stats.h's workgroup sum) and writes
//                         the four values.
//
// Every operation after the fp32 loads is fp64.  No atomics: a workgroup's three sums (stats.h's workgroup sum) go to the
// workspace with plain vector stores, so a call is reproducible bit for bit; nothing is allocated, copied or synchronised here.
#include <cfloat>

#include "stats.h"

namespace {

constexpr int TH = 16, TW = 32, NT = 128;         // tile of a workgroup; lane t owns row t / 8, columns 4 (t % 8) .. + 3
constexpr int HALO = 2, PADX = 4;                 // rows / columns staged around the tile (columns: a whole float4)
constexpr int LH = TH + 2 * HALO, LS = TW + 2 * PADX;   // staged tile: 20 x 40 floats; column x0 - PADX + lx
constexpr int SH = TH + 2, SW = TW + 2, SS = 36;  // sign map: the tile and a halo of 1, row stride 36
constexpr int MAXC = 16, FIN_T = 256;

inline long tiles_of(int H, int W) { return (long)((H + TH - 1) / TH) * ((W + TW - 1) / TW); }

struct LossArgs {
  const float* x0;
  const float* xh;
  const float* ms;   // null when do_sam == 0
  float* g;          // null: values only
  int C, H, W, tiles_x, tiles, base_kind, vec, do_sam, do_lap;
  double gb, gs, gl;   // gradient scales: 1 / (B C H W), w_sam / (B H W), w_lap / (B C (H - 2)(W - 2))
  double* part;        // [workgroups][3]: sum rho, sum angle, sum |Lap d|
};

// the lane's four pixels of one plane (zeros outside the image)
__device__ __forceinline__ void load_quad(const float* __restrict__ p, long off, int gx, int W, bool row_in, bool vec, float (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (!row_in || gx >= W) return;
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(p + off);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (gx + j < W) v[j] = p[off + j];
  }
}

__global__ void __launch_bounds__(NT) loss_kernel(LossArgs p) {
  __shared__ __attribute__((aligned(16))) float sa[LH][LS];   // x0
  __shared__ __attribute__((aligned(16))) float sb[LH][LS];   // xh
  __shared__ float ss[SH][SS];                                // sign(Lap d), 0 outside the interior
  __shared__ double red[NT / 64][3];

  const int t = threadIdx.x, row = t >> 3, qx = (t & 7) * 4;
  const int img = blockIdx.x / p.tiles, tile = blockIdx.x - img * p.tiles;
  const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
  const int y0 = ty * TH, x0 = tx * TW;
  const int H = p.H, W = p.W, C = p.C;
  const int gy = y0 + row, gx = x0 + qx;
  const bool row_in = gy < H, vec = p.vec != 0;
  const long plane = (long)H * W, ibase = (long)img * C * plane, own = (long)gy * W + gx;

  double s_base = 0.0, s_sam = 0.0, s_lap = 0.0;
  double ca[4] = {0.0, 0.0, 0.0, 0.0}, cb[4] = {0.0, 0.0, 0.0, 0.0};   // sam gradient of band c: ca * u_c + cb * v_c

  if (p.do_sam) {
    double dot[4] = {0.0, 0.0, 0.0, 0.0}, nu[4] = {0.0, 0.0, 0.0, 0.0}, nv[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < C; ++c) {
      const long off = ibase + c * plane + own;
      float a[4], b[4], m[4];
      load_quad(p.x0, off, gx, W, row_in, vec, a);
      load_quad(p.xh, off, gx, W, row_in, vec, b);
      load_quad(p.ms, off, gx, W, row_in, vec, m);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double u = (double)a[j] + (double)m[j], v = (double)b[j] + (double)m[j];
        dot[j] += u * v; nu[j] += u * u; nv[j] += v * v;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (row_in && gx + j < W) {
#pragma clang fp contract(off)   // the two products round separately, as the host definition's do
        const double cr2 = nu[j] * nv[j] - dot[j] * dot[j];
        const bool ok = C > 1 && nu[j] > 0.0 && nv[j] > 0.0 && cr2 > 0.0;   // one band: u and v are parallel whatever rounding says
        const double cr = ok ? sqrt(cr2) : 0.0;
        s_sam += atan2(cr, dot[j]);
        if (ok) {
          ca[j] = -p.gs / cr;
          cb[j] = p.gs * dot[j] / (nv[j] * cr);
        }
      }
    }
  }

  for (int c = 0; c < C; ++c) {
    const long cbase = ibase + c * plane;
    const float* pa = p.x0 + cbase;
    const float* pb = p.xh + cbase;
    float a[4], b[4];
    double glap[4] = {0.0, 0.0, 0.0, 0.0};
    if (p.do_lap) {
      __syncthreads();   // the previous band's readers are done
      tmdiff::stage_halo_tile<float, LH, LS, LS, NT>(sa[0], sb[0], pa, pb, nullptr, y0 - HALO, x0 - PADX, H, W, vec);
      __syncthreads();
      for (int i = t; i < SH * SW; i += NT) {
        const int sy = i / SW, sx = i - sy * SW;
        const int py = y0 - 1 + sy, px = x0 - 1 + sx;
        float sg = 0.f;
        if (py >= 1 && py <= H - 2 && px >= 1 && px <= W - 2) {
          const int ly = sy + 1, lx = sx + (PADX - 1);
          double nb = 0.0;
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
              if (dy != 0 || dx != 0) nb += (double)sb[ly + dy][lx + dx] - (double)sa[ly + dy][lx + dx];
          const double lap = nb - 8.0 * ((double)sb[ly][lx] - (double)sa[ly][lx]);
          sg = lap > 0.0 ? 1.f : lap < 0.0 ? -1.f : 0.f;
          if (sy >= 1 && sy <= TH && sx >= 1 && sx <= TW) s_lap += fabs(lap);
        }
        if (p.g) ss[sy][sx] = sg;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] = sa[row + HALO][qx + PADX + j];
        b[j] = sb[row + HALO][qx + PADX + j];
        if (p.g) {
          float nb = 0.f;   // sums of at most nine values of -1, 0, 1: exact
#pragma unroll
          for (int dy = 0; dy <= 2; ++dy)
#pragma unroll
            for (int dx = 0; dx <= 2; ++dx) nb += ss[row + dy][qx + j + dx];
          glap[j] = p.gl * (double)(nb - 9.f * ss[row + 1][qx + j + 1]);
        }
      }
    } else {
      load_quad(pa, own, gx, W, row_in, vec, a);
      load_quad(pb, own, gx, W, row_in, vec, b);
    }
    float m[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.do_sam && p.g) load_quad(p.ms, cbase + own, gx, W, row_in, vec, m);

    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      out[j] = 0.f;
      if (row_in && gx + j < W) {
        const double d = (double)b[j] - (double)a[j], ad = fabs(d);
        const double sgn = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : 0.0;
        double rho, drho;
        if (p.base_kind == 0) rho = ad, drho = sgn;
        else if (p.base_kind == 1) rho = d * d, drho = 2.0 * d;
        else if (ad < 1.0) rho = 0.5 * d * d, drho = d;
        else rho = ad - 0.5, drho = sgn;
        s_base += rho;
        const double u = (double)a[j] + (double)m[j], v = (double)b[j] + (double)m[j];
        const double gd = p.gb * drho + glap[j] + (ca[j] * u + cb[j] * v);
        out[j] = fminf(fmaxf((float)gd, -FLT_MAX), FLT_MAX);   // 1 / |v| can pass the fp32 range: saturate, never inf
      }
    }
    if (p.g && row_in && gx < W) {
      float* pg = p.g + cbase + own;
      if (vec) {
        *reinterpret_cast<float4*>(pg) = make_float4(out[0], out[1], out[2], out[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (gx + j < W) pg[j] = out[j];
      }
    }
  }

  const double s[3] = {s_base, s_sam, s_lap};
  tmdiff::wg_sum_store<3, 3>(s, red[0]);
  __syncthreads();
  if (t < 3) p.part[(long)blockIdx.x * 3 + t] = tmdiff::wg_sum_col<NT / 64, 3>(red[0], t);
}

struct LossFinalArgs {
  const double* part;
  long n;                 // workgroups
  double nb, ns, nl;      // counts of the three means (nl = 0: no interior)
  double w_sam, w_lap;
  double* out64;          // total, base, sam, lap
  float* out32;           // total
};

// Lane t adds the workgroups t, t + 256, ... in order, then the workgroup sum: the order depends on the number of workgroups alone.
__global__ void __launch_bounds__(FIN_T) loss_finalize_kernel(LossFinalArgs p) {
  __shared__ double red[FIN_T / 64][3];
  const int t = threadIdx.x;
  double s[3] = {0.0, 0.0, 0.0};
  for (long i = t; i < p.n; i += FIN_T) {   // stats.h strided_sum's walk over the three columns at once: their loads overlap
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += p.part[i * 3 + k];
  }
  tmdiff::wg_sum_store<3, 3>(s, red[0]);
  __syncthreads();
  if (t != 0) return;
  double tot[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) tot[k] = tmdiff::wg_sum_col<FIN_T / 64, 3>(red[0], k);
  const double base = tot[0] / p.nb, sam = tot[1] / p.ns, lap = p.nl > 0.0 ? tot[2] / p.nl : 0.0;
  double total;
  {
#pragma clang fp contract(off)   // (base + w_sam * sam) + w_lap * lap with every operation rounded, as the host writes it
    total = base + p.w_sam * sam + p.w_lap * lap;
  }
  p.out64[0] = total; p.out64[1] = base; p.out64[2] = sam; p.out64[3] = lap;
  *p.out32 = (float)total;
}

bool loss_ok(int B, int C, int H, int W, int lap) {
  const int least = lap ? 3 : 1;
  return B >= 1 && C >= 1 && C <= MAXC && H >= least && W >= least && tmdiff::fits_int32((double)B * C * H * W);
}

size_t loss_bytes(int B, int H, int W) { return (size_t)B * tiles_of(H, W) * 3 * sizeof(double); }

}  // namespace

extern "C" {

int tmdiff_loss_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t lap) {
  return loss_ok(B, C, H, W, lap);   // a predicate: it leaves the last-error string alone
}

size_t tmdiff_loss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t lap) {
  return loss_ok(B, C, H, W, lap) ? loss_bytes(B, H, W) : 0;
}

int tmdiff_spectral_spatial_loss(const float* x0, const float* xhat, const float* ms, float* g, int32_t base_kind, double w_sam,
                                 double w_lap, double* out64, float* out32, void* workspace, size_t workspace_bytes, int32_t B,
                                 int32_t C, int32_t H, int32_t W, tmdiff_stream_t stream) {
  TMDIFF_REQUIRE(base_kind >= 0 && base_kind <= 2, "spectral_spatial_loss: base_kind=%d (0 = l1, 1 = l2, 2 = smooth_l1)", base_kind);
  TMDIFF_REQUIRE(w_sam >= 0.0 && w_lap >= 0.0 && w_sam <= DBL_MAX && w_lap <= DBL_MAX,
                 "spectral_spatial_loss: w_sam=%g w_lap=%g (finite, not negative)", w_sam, w_lap);
  const int lap = w_lap != 0.0;
  if (!loss_ok(B, C, H, W, lap))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "spectral_spatial_loss: B=%d C=%d H=%d W=%d (B >= 1, 1 <= C <= 16, H, W >= %d, fewer than "
                        "2^31 elements)", B, C, H, W, lap ? 3 : 1);
  TMDIFF_REQUIRE(x0 && xhat && out64 && out32 && workspace, "spectral_spatial_loss: null tensor");
  TMDIFF_REQUIRE(ms || w_sam == 0.0, "spectral_spatial_loss: ms may be null only when w_sam == 0");
  if (const int rc = tmdiff::check_workspace("spectral_spatial_loss", workspace, workspace_bytes, loss_bytes(B, H, W), ", as out64", out64))
    return rc;
  const hipStream_t st = tmdiff::as_stream(stream);
  const int tiles_x = (W + TW - 1) / TW;
  const long tiles = tiles_of(H, W), blocks = (long)B * tiles;
  if (const int rc = tmdiff::check_grid(blocks, "spectral_spatial_loss", TMDIFF_E_UNSUPPORTED)) return rc;
  const bool sam = w_sam != 0.0;
  const bool vec = W % 4 == 0 && tmdiff::aligned16(x0) && tmdiff::aligned16(xhat) && (!sam || tmdiff::aligned16(ms)) &&
                   (!g || tmdiff::aligned16(g));
  const double nb = (double)B * C * H * W, ns = (double)B * H * W, nl = lap ? (double)B * C * (H - 2) * (W - 2) : 0.0;
  const LossArgs a{x0, xhat, sam ? ms : nullptr, g, C, H, W, tiles_x, (int)tiles, base_kind, vec, sam, lap,
                   1.0 / nb, w_sam / ns, lap ? w_lap / nl : 0.0, static_cast<double*>(workspace)};
  loss_kernel<<<(unsigned)blocks, NT, 0, st>>>(a);
  if (const int rc = tmdiff::check_launch("spectral_spatial_loss")) return rc;
  const LossFinalArgs f{a.part, blocks, nb, ns, nl, w_sam, w_lap, out64, out32};
  loss_finalize_kernel<<<1, FIN_T, 0, st>>>(f);
  return tmdiff::check_launch("spectral_spatial_loss (finalize)");
}

}  // extern "C"

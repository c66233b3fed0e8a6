// Overlapped scene tiles for fused ("MultiDiffusion") sampling on gfx950: cut tiles out of one scene (gather) and blend tile
// predictions back into one scene (blend).  Both are HBM-bound copies: 16 bytes per lane along W where the plan allows it,
// plain vector stores, no LDS, no atomics (tmdiff_amd/tiling.py; the reference tiles without overlap, data/LRHR_dataset.py:17-53).
//
// The plan per axis of length L: origins 0, s, 2s, ... (s = tile - overlap) while origin + tile <= L, and one more tile pushed
// inwards to L - tile when the last regular one does not end at L.  In closed form origin(i) = min(i * s, L - tile), so the
// kernels need no origin table.  With overlap <= tile / 2 a pixel lies in at most two regular tiles per axis, and the pushed-in
// one can be a third: the tiles that cover coordinate p are among p / s - 1, p / s, p / s + 1.
// 1-D weight of tile-local coordinate i: min(i + 1, tile - i, overlap + 1) (a ramp of `overlap` pixels at either end); a tile's
// 2-D weight is the product and a scene pixel is sum(w v) / sum(w) over its covering tiles, visited in row-major order.
#include <algorithm>

#include "common.h"

namespace {

struct TilePlan {
  int H, W, C, tile, overlap, step, ny, nx;
};

__host__ __device__ __forceinline__ int tile_count(int L, int tile, int step) {
  return (L - tile) / step + 1 + ((L - tile) % step != 0);
}
__host__ __device__ __forceinline__ int tile_origin(int i, int step, int L, int tile) {
  const int o = i * step;
  return o < L - tile ? o : L - tile;
}
__device__ __forceinline__ float tile_w1(int i, int tile, int overlap) { return (float)min(min(i + 1, tile - i), overlap + 1); }

// tiles[(b * ny * nx + iy * nx + ix), c, ty, tx] = scene[b, c, oy(iy) + ty, ox(ix) + tx].  One lane per V outputs; blockIdx.y
// walks the tile planes (n, c), whose decode is wave-uniform.
template <int V>
__global__ void __launch_bounds__(256) tile_gather_kernel(const float* __restrict__ scene, float* __restrict__ tiles, TilePlan p,
                                                          int planes) {
  const int tv = p.tile / V;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= p.tile * tv) return;
  const int ty = g / tv, tx = (g - ty * tv) * V;
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const int n = pl / p.C, c = pl - n * p.C;
    const int b = n / (p.ny * p.nx), r = n - b * (p.ny * p.nx);
    const int iy = r / p.nx, ix = r - iy * p.nx;
    const int src = ((b * p.C + c) * p.H + tile_origin(iy, p.step, p.H, p.tile) + ty) * p.W + tile_origin(ix, p.step, p.W, p.tile) + tx;
    const int dst = (pl * p.tile + ty) * p.tile + tx;
    if constexpr (V == 4)
      *reinterpret_cast<float4*>(tiles + dst) = *reinterpret_cast<const float4*>(scene + src);
    else
      tiles[dst] = scene[src];
  }
}

// scene[b, c, y, x] = sum_t w_t v_t / sum_t w_t over the tiles t that cover (y, x), rows of tiles outside, columns inside
// (row-major tile order).  One lane owns V neighbouring pixels of a scene row; in the 16-byte form all column origins and the
// tile edge are multiples of 4, so a tile covers all four pixels of a lane or none.  blockIdx.y walks the scene planes (b, c).
template <int V>
__global__ void __launch_bounds__(256) tile_blend_kernel(const float* __restrict__ tiles, float* __restrict__ scene, TilePlan p,
                                                         int planes) {
  const int wv = p.W / V;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= p.H * wv) return;
  const int y = g / wv, x = (g - y * wv) * V;
  const int ky = y / p.step, kx = x / p.step;
  const int iy0 = max(ky - 1, 0), iy1 = min(ky + 1, p.ny - 1), ix0 = max(kx - 1, 0), ix1 = min(kx + 1, p.nx - 1);
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const int b = pl / p.C, c = pl - b * p.C;
    float acc[V], den[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = den[j] = 0.f;
    for (int iy = iy0; iy <= iy1; ++iy) {
      const int ty = y - tile_origin(iy, p.step, p.H, p.tile);
      if (ty < 0 || ty >= p.tile) continue;
      const float wy = tile_w1(ty, p.tile, p.overlap);
      for (int ix = ix0; ix <= ix1; ++ix) {
        const int tx = x - tile_origin(ix, p.step, p.W, p.tile);
        if (tx < 0 || tx >= p.tile) continue;
        const int src = ((((b * p.ny + iy) * p.nx + ix) * p.C + c) * p.tile + ty) * p.tile + tx;
        float v[V];
        if constexpr (V == 4)
          *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(tiles + src);
        else
          v[0] = tiles[src];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float w = __fmul_rn(wy, tile_w1(tx + j, p.tile, p.overlap));   // small integers: exact
          acc[j] = fmaf(w, v[j], acc[j]);
          den[j] = __fadd_rn(den[j], w);
        }
      }
    }
    float o[V];
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = __fdiv_rn(acc[j], den[j]);   // every pixel is covered: den >= 1
    const int dst = (pl * p.H + y) * p.W + x;
    if constexpr (V == 4)
      *reinterpret_cast<float4*>(scene + dst) = *reinterpret_cast<float4*>(o);
    else
      scene[dst] = o[0];
  }
}

int check_plan(const char* what, int B, int C, int H, int W, int tile, int overlap) {
  TMDIFF_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0, "%s: bad extents B=%d C=%d H=%d W=%d", what, B, C, H, W);
  TMDIFF_REQUIRE(tile > 0 && tile <= H && tile <= W, "%s: tile=%d does not fit a %d x %d scene", what, tile, H, W);
  TMDIFF_REQUIRE(overlap >= 0 && overlap <= tile / 2, "%s: overlap=%d (0 <= overlap <= tile / 2 = %d)", what, overlap, tile / 2);
  return TMDIFF_OK;
}

// 32-bit element offsets: the scene and the tile stack must each hold fewer than 2^31 elements
bool offsets_fit(int B, int C, int H, int W, int tile, int overlap) {
  const int step = tile - overlap;
  const double nt = (double)B * tile_count(H, tile, step) * tile_count(W, tile, step);
  return (double)B * C * H * W <= 2147483647.0 && nt * C * tile * tile <= 2147483647.0;
}

template <bool BLEND>
int launch(const char* what, const float* in, float* out, int B, int C, int H, int W, int tile, int overlap, tmdiff_stream_t stream) {
  if (const int rc = check_plan(what, B, C, H, W, tile, overlap)) return rc;
  if (B == 0) return TMDIFF_OK;
  TMDIFF_REQUIRE(in && out, "%s: null tensor", what);
  if (!offsets_fit(B, C, H, W, tile, overlap))
    return tmdiff::fail(TMDIFF_E_UNSUPPORTED, "%s: B=%d C=%d H=%d W=%d tile=%d overlap=%d exceeds 32-bit element offsets", what, B, C, H,
                        W, tile, overlap);
  const int step = tile - overlap;
  const TilePlan p{H, W, C, tile, overlap, step, tile_count(H, tile, step), tile_count(W, tile, step)};
  // 16-byte form: every row start and every column origin (multiples of step, and W - tile) on a 4-element boundary
  const bool vec = W % 4 == 0 && tile % 4 == 0 && step % 4 == 0 && tmdiff::aligned16(in) && tmdiff::aligned16(out);
  const int planes = BLEND ? B * C : B * p.ny * p.nx * C;
  const long per_plane = BLEND ? (long)H * (W / (vec ? 4 : 1)) : (long)tile * (tile / (vec ? 4 : 1));
  const dim3 grid((unsigned)((per_plane + 255) / 256), (unsigned)std::min(planes, 65535));
  const hipStream_t st = tmdiff::as_stream(stream);
  if constexpr (BLEND) {
    if (vec) tile_blend_kernel<4><<<grid, 256, 0, st>>>(in, out, p, planes);
    else tile_blend_kernel<1><<<grid, 256, 0, st>>>(in, out, p, planes);
  } else {
    if (vec) tile_gather_kernel<4><<<grid, 256, 0, st>>>(in, out, p, planes);
    else tile_gather_kernel<1><<<grid, 256, 0, st>>>(in, out, p, planes);
  }
  return tmdiff::check_launch(what);
}

}  // namespace

extern "C" {

int32_t tmdiff_tile_plan(int32_t L, int32_t tile, int32_t overlap, int32_t* origins, int32_t capacity) {
  if (L <= 0 || tile <= 0 || tile > L || overlap < 0 || overlap > tile / 2) {
    tmdiff::fail(TMDIFF_E_INVALID, "tile_plan: L=%d tile=%d overlap=%d (need tile <= L, 0 <= overlap <= tile / 2)", L, tile, overlap);
    return -1;
  }
  const int step = tile - overlap, n = tile_count(L, tile, step);
  for (int i = 0; origins && i < n && i < capacity; ++i) origins[i] = tile_origin(i, step, L, tile);
  return n;
}

int tmdiff_tile_supported(int32_t B, int32_t C, int32_t H, int32_t W, int32_t tile, int32_t overlap) {
  // a predicate: it leaves the last-error string alone
  const bool plan_ok = B >= 0 && C > 0 && H > 0 && W > 0 && tile > 0 && tile <= H && tile <= W && overlap >= 0 && overlap <= tile / 2;
  return plan_ok && offsets_fit(B, C, H, W, tile, overlap);
}

int tmdiff_tile_gather(const float* scene, float* tiles, int32_t B, int32_t C, int32_t H, int32_t W, int32_t tile, int32_t overlap,
                       tmdiff_stream_t stream) {
  return launch<false>("tile_gather", scene, tiles, B, C, H, W, tile, overlap, stream);
}

int tmdiff_tile_blend(const float* tiles, float* scene, int32_t B, int32_t C, int32_t H, int32_t W, int32_t tile, int32_t overlap,
                      tmdiff_stream_t stream) {
  return launch<true>("tile_blend", tiles, scene, B, C, H, W, tile, overlap, stream);
}

}  // extern "C"

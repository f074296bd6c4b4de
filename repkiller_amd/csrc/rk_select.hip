// rk_select.hip -- result rows selected by repeat flag (rk_result_select,
// rk_batch_result_select): a stable segmented stream compaction of the triple
// (out_order, gid, repval) in rk_batch_result layout.  The predicate and the
// destination arithmetic are rk_select.h's, shared with the host selection.
//
// A tile is T = 4096 slots, one 256-thread block, 16 slots (one 16-B word of
// flags) per lane:
//   1. count pass: the tile's kept count and its used slots by flag;
//   2. k_csv_scan<uint64_t> of the tile counts (rk_csv_scan.h);
//   3. set bases: one wave per entry of off[] evaluates the exclusive kept
//      prefix there (tile offset + the kept flags before it in its tile); the
//      last block sums the tiles' by-flag counts.  No atomics anywhere;
//   4. scatter pass: the block ranks its kept slots, stages destination, flag
//      and (one array after the other) value of each in LDS in rank order, and
//      writes them with consecutive lanes on consecutive words.
// One upload (the set table) and one readback (the bases and the counts) per
// call; scratch from ctx->ws, everything on ctx->stream.
#include <algorithm>
#include <new>

#include "rk_csv_scan.h"
#include "rk_ctx.h"
#include "rk_select.h"

namespace {

using rk::SelCur;
using rk::SelTab;

constexpr uint32_t ST = 256;                  // threads of a block
constexpr uint32_t T = ST * rk::SEL_GROUP;    // slots of a tile
constexpr uint32_t WAVES = ST / 64;

struct Res3 {
  const uint32_t *order, *gid;
  const uint8_t *rep;
};
struct Out3 {
  uint32_t *order, *gid;
  uint8_t *rep;
};

__device__ inline uint32_t wave_sum(uint32_t v) {
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// exclusive scan of v over the block's ST threads, one barrier: a shuffle scan
// in every wave, then the waves' totals through wsum[WAVES]
__device__ inline uint32_t block_scan(uint32_t v, uint32_t *wsum, uint32_t *total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t incl = v;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63u) wsum[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t k = 0; k < WAVES; ++k) {
    const uint32_t x = wsum[k];
    before += k < wave ? x : 0u;
    all += x;
  }
  *total = all;
  return before + incl - v;
}

// Kept bits of the group of up to 16 slots at p0 < lim (p0 a multiple of 16):
// the flags come as one 16-B word where the array allows it.  The set of
// wave_p, the first slot of the wave's groups, is searched at a wave-uniform
// address; the lane searches on only when its group starts past that set's end.
// *c0: the cursor at the group's start; w: the flags.
__device__ inline uint32_t group_mask(const SelTab &tab, const uint8_t *rep, uint64_t lim,
                                      uint64_t p0, uint64_t wave_p, uint32_t keep, uint32_t w[4],
                                      SelCur *c0, uint32_t *by) {
  const uint32_t cnt = (uint32_t)min((uint64_t)rk::SEL_GROUP, lim - p0);
  if (cnt == rk::SEL_GROUP && ((uintptr_t)rep & 15u) == 0) {
    const uint4 v = *reinterpret_cast<const uint4 *>(rep + p0);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (uint32_t j = 0; j < rk::SEL_GROUP; ++j)
      if (j < cnt) w[j >> 2] |= (uint32_t)rep[p0 + j] << (8u * (j & 3u));
  }
  SelCur c;
  rk::sel_load(tab, c, rk::sel_set_of(tab, 0, wave_p));
  rk::sel_seek(tab, c, p0);
  *c0 = c;
  return rk::sel_mask(tab, c, p0, cnt, w, keep, by);
}

__global__ __launch_bounds__(ST) void k_sel_count(SelTab tab, const uint8_t *rep, uint64_t n,
                                                 uint32_t keep, uint32_t *tile_cnt,
                                                 uint4 *tile_by) {
  __shared__ uint32_t red[WAVES][3];
  const uint32_t t = threadIdx.x;
  const uint64_t tile0 = (uint64_t)blockIdx.x * T, p0 = tile0 + t * rk::SEL_GROUP;
  uint32_t m = 0, by = 0;
  if (p0 < n) {
    uint32_t w[4];
    SelCur c;
    m = group_mask(tab, rep, n, p0, tile0 + (t & ~63u) * rk::SEL_GROUP, keep, w, &c, &by);
  }
  // (a wave's fields reach 1024, a block's 4096: two 16-bit fields per word)
  const uint32_t k = wave_sum(__popc(m)), lo = wave_sum(by & 0x00FF00FFu),
                 hi = wave_sum((by >> 8) & 0x00FF00FFu);
  if ((t & 63u) == 0) red[t >> 6][0] = k, red[t >> 6][1] = lo, red[t >> 6][2] = hi;
  __syncthreads();
  if (t == 0) {
    uint32_t a = 0, b = 0, c = 0;
    for (uint32_t v = 0; v < WAVES; ++v) a += red[v][0], b += red[v][1], c += red[v][2];
    tile_cnt[blockIdx.x] = a;
    tile_by[blockIdx.x] = make_uint4(b & 0xFFFFu, c & 0xFFFFu, b >> 16, c >> 16);
  }
}

// base[e] = kept slots before off[e], e <= ns, one wave each; the last block:
// by_out[0..3] = the used slots by flag, over all tiles
__global__ __launch_bounds__(ST) void k_sel_bases(SelTab tab, const uint8_t *rep, uint32_t keep,
                                                 const uint64_t *tile_off, const uint4 *tile_by,
                                                 uint32_t nb, uint64_t *base,
                                                 unsigned long long *by_out) {
  __shared__ unsigned long long red[ST][4];
  const uint32_t t = threadIdx.x, lane = t & 63u;
  if (blockIdx.x == gridDim.x - 1) {
    unsigned long long a[4] = {0, 0, 0, 0};
    for (uint32_t i = t; i < nb; i += ST) {
      const uint4 v = tile_by[i];
      a[0] += v.x, a[1] += v.y, a[2] += v.z, a[3] += v.w;
    }
    for (int f = 0; f < 4; ++f) red[t][f] = a[f];
    __syncthreads();
    for (uint32_t d = ST / 2; d; d >>= 1) {
      if (t < d)
        for (int f = 0; f < 4; ++f) red[t][f] += red[t + d][f];
      __syncthreads();
    }
    if (t < 4) by_out[t] = red[0][t];
    return;
  }
  const uint32_t e = blockIdx.x * WAVES + (t >> 6);
  if (e > tab.ns) return;
  const uint64_t p = tab.off[e], b = p / T, tile0 = b * T;
  uint32_t sum = 0;
  for (uint64_t g0 = 0; tile0 + g0 * rk::SEL_GROUP < p; g0 += 64) {
    const uint64_t p0 = tile0 + (g0 + lane) * rk::SEL_GROUP;
    if (p0 < p) {
      uint32_t w[4], by = 0;
      SelCur c;
      sum += __popc(group_mask(tab, rep, p, p0, tile0 + g0 * rk::SEL_GROUP, keep, w, &c, &by));
    }
  }
  sum = wave_sum(sum);
  if (lane == 0) base[e] = tile_off[b] + sum;
}

__global__ __launch_bounds__(ST) void k_sel_scatter(SelTab tab, Res3 in, uint64_t n, uint32_t keep,
                                                   const uint64_t *tile_off, const uint64_t *base,
                                                   Out3 out) {
  __shared__ uint32_t s_val[T], s_dst[T];
  __shared__ __attribute__((aligned(4))) uint8_t s_rep[T];
  __shared__ uint32_t s_wsum[WAVES], s_mask[ST], s_rank[ST];
  const uint32_t t = threadIdx.x;
  const uint64_t tile0 = (uint64_t)blockIdx.x * T, p0 = tile0 + t * rk::SEL_GROUP;
  uint32_t m = 0, by = 0, w[4] = {0, 0, 0, 0};
  SelCur c{};
  if (p0 < n) m = group_mask(tab, in.rep, n, p0, tile0 + (t & ~63u) * rk::SEL_GROUP, keep, w, &c, &by);
  uint32_t total;
  const uint32_t rank = block_scan(__popc(m), s_wsum, &total);
  if (total == 0) return;  // (the whole block)
  s_mask[t] = m, s_rank[t] = rank;
  if (m) {
    // destination and flag of the lane's kept slots, in rank order
    const uint64_t tbase = tile_off[blockIdx.x];
    uint32_t r = rank, cs = ~0u;
    uint64_t cb = 0;
#pragma unroll
    for (uint32_t j = 0; j < rk::SEL_GROUP; ++j) {
      if ((m >> j) & 1u) {
        rk::sel_seek(tab, c, p0 + j);
        if (c.s != cs) cs = c.s, cb = base[cs];
        s_dst[r] = (uint32_t)rk::sel_dst(c.lo, cb, tbase + r);
        s_rep[r] = (uint8_t)rk::sel_flag(w, j);
        ++r;
      }
    }
  }
  __syncthreads();
  // the two 4-B arrays, one after the other through s_val: consecutive lanes
  // read consecutive slots (16-B words in a full tile of 16-B aligned arrays)
  // and write consecutive destinations (one run per set)
  const bool vec = tile0 + T <= n && (((uintptr_t)in.order | (uintptr_t)in.gid) & 15u) == 0;
  for (int a = 0; a < 2; ++a) {
    const uint32_t *src = a ? in.gid : in.order;
    uint32_t *dst = a ? out.gid : out.order;
    if (vec) {
#pragma unroll
      for (uint32_t i = 0; i < rk::SEL_GROUP / 4; ++i) {
        const uint32_t q = (i * ST + t) * 4u, own = q / rk::SEL_GROUP, bit = q % rk::SEL_GROUP;
        const uint32_t mo = s_mask[own], nib = (mo >> bit) & 15u;
        if (nib) {
          const uint4 v = *reinterpret_cast<const uint4 *>(src + tile0 + q);
          uint32_t r = s_rank[own] + __popc(mo & ((1u << bit) - 1u));
          if (nib & 1u) s_val[r++] = v.x;
          if (nib & 2u) s_val[r++] = v.y;
          if (nib & 4u) s_val[r++] = v.z;
          if (nib & 8u) s_val[r] = v.w;
        }
      }
    } else {
#pragma unroll 4
      for (uint32_t i = 0; i < rk::SEL_GROUP; ++i) {
        const uint32_t q = i * ST + t, own = q / rk::SEL_GROUP, bit = q % rk::SEL_GROUP;
        const uint32_t mo = s_mask[own];
        if ((mo >> bit) & 1u)
          s_val[s_rank[own] + __popc(mo & ((1u << bit) - 1u))] = src[tile0 + q];
      }
    }
    __syncthreads();
    for (uint32_t r = t; r < total; r += ST) dst[s_dst[r]] = s_val[r];
    __syncthreads();
  }
  // the flags: a tile whose destinations are one run writes them as dwords
  const uint32_t d0 = s_dst[0];
  if (s_dst[total - 1] - d0 == total - 1) {
    uint8_t *o = out.rep + d0;
    const uint32_t head = min(total, (uint32_t)((4u - ((uintptr_t)o & 3u)) & 3u));
    const uint32_t nw = (total - head) / 4u;
    if (t < head) o[t] = s_rep[t];
    for (uint32_t v = t; v < nw; v += ST) {
      const uint32_t k = head + 4u * v;
      *reinterpret_cast<uint32_t *>(o + k) = (uint32_t)s_rep[k] | (uint32_t)s_rep[k + 1] << 8 |
                                             (uint32_t)s_rep[k + 2] << 16 |
                                             (uint32_t)s_rep[k + 3] << 24;
    }
    for (uint32_t k = head + 4u * nw + t; k < total; k += ST) o[k] = s_rep[k];
  } else {
    for (uint32_t r = t; r < total; r += ST) out.rep[s_dst[r]] = s_rep[r];
  }
}

// ------------------------------------------------------------------ host --

int check_table(uint32_t ns, const uint64_t *off, const uint64_t *n_out) {
  for (uint32_t k = 0; k < ns; ++k)
    if (off[k + 1] < off[k] || n_out[k] > off[k + 1] - off[k]) return RK_E_ARG;
  return RK_OK;
}

bool valid_keep(uint32_t keep) { return keep >= 1 && keep <= (uint32_t)RK_KEEP_ALL; }

void put_stats(rk_ctx *ctx, uint32_t ns, const uint64_t *n_out, const uint64_t *kept,
               const uint64_t by[4], double ms) {
  if (!ctx) return;
  rk_select_stats &st = ctx->select;
  st = rk_select_stats{};
  for (uint32_t k = 0; k < ns; ++k) st.rows_in += n_out[k], st.kept += kept[k];
  for (int f = 0; f < 4; ++f) st.by_flag[f] = by[f];
  st.sets = ns;
  st.device_ms = ms;
}

template <class F>
int guarded(rk_ctx *ctx, F &&body) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    if (ctx) {
      if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
      ctx->err = "select: out of host memory";
    }
    return RK_E_NOMEM;
  } catch (...) {
    if (ctx) ctx->err = "unexpected C++ exception";
    return RK_E_INTERNAL;
  }
}

// the selection of one validated table; host arrays, or device arrays on ctx
int select_any(rk_ctx *ctx, uint32_t ns, const uint64_t *off, const uint64_t *n_out,
               const uint32_t *order, const uint32_t *gid, const uint8_t *rep, uint32_t keep,
               uint32_t flags, uint32_t *o_order, uint32_t *o_gid, uint8_t *o_rep,
               uint64_t *kept) {
  if (flags & RK_RES_DEVICE)
    return rk::select_device(ctx, ns, off, n_out, order, gid, rep, keep, o_order, o_gid, o_rep,
                             kept);
  uint64_t by[4] = {0, 0, 0, 0}, rows = 0;
  for (uint32_t k = 0; k < ns; ++k) kept[k] = 0, rows += n_out[k];
  if (rows)  // (without rows the arrays may be null)
    rk::select_host(SelTab{off, n_out, ns}, order, gid, rep, keep, o_order, o_gid, o_rep, kept, by);
  put_stats(ctx, ns, n_out, kept, by, 0.0);
  return RK_OK;
}

}  // namespace

int rk::select_device(rk_ctx *ctx, uint32_t ns, const uint64_t *off, const uint64_t *n_out,
                      const uint32_t *order, const uint32_t *gid, const uint8_t *rep,
                      uint32_t keep, uint32_t *o_order, uint32_t *o_gid, uint8_t *o_rep,
                      uint64_t *kept) {
  // the kernels see the table from slot 0: a first offset above zero moves the
  // arrays instead (slots before off[0] belong to no set)
  const uint64_t first = ns ? off[0] : 0;
  order += first, gid += first, rep += first;
  o_order += first, o_gid += first, o_rep += first;
  const uint64_t n = ns ? off[ns] - first : 0;
  uint64_t rows = 0;
  for (uint32_t k = 0; k < ns; ++k) kept[k] = 0, rows += n_out[k];
  if (!rows) {
    const uint64_t none[4] = {0, 0, 0, 0};
    put_stats(ctx, ns, n_out, kept, none, 0.0);
    return RK_OK;
  }
  if (n > 0xFFFFFFFFull) {
    ctx->err = "select: more than 2^32 - 1 slots";
    return RK_E_TOO_MANY;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint32_t nb = (uint32_t)((n + T - 1) / T);
  // scratch: tile arrays; down = base[ns + 1] + by[4]; up = off[ns + 1] + n_out[ns]
  uint32_t *tile_cnt;
  uint4 *tile_by;
  uint64_t *tile_off, *down, *up;
  auto carve = [&](rk::Carve &c) {
    tile_cnt = c.take<uint32_t>(nb), tile_by = c.take<uint4>(nb);
    tile_off = c.take<uint64_t>((size_t)nb + 1);
    down = c.take<uint64_t>((size_t)ns + 5), up = c.take<uint64_t>(2 * (size_t)ns + 1);
  };
  rk::Carve size{nullptr};
  carve(size);
  int rc = rk::grow(ctx, &ctx->ws, &ctx->ws_cap, size.off, "select scratch");
  if (rc) return rc;
  rk::Carve place{(char *)ctx->ws};
  carve(place);

  std::vector<uint64_t> hup(2 * (size_t)ns + 1), hdown((size_t)ns + 5);
  for (uint32_t k = 0; k <= ns; ++k) hup[k] = off[k] - first;
  std::copy(n_out, n_out + ns, hup.begin() + ns + 1);
  const SelTab tab{up, up + ns + 1, ns};
  uint64_t *base = down;
  unsigned long long *by = reinterpret_cast<unsigned long long *>(down + ns + 1);
  hipStream_t s = ctx->stream;
  HIPCHK(ctx, hipEventRecord(ctx->ev0, s));
  HIPCHK(ctx, hipMemcpyAsync(up, hup.data(), hup.size() * 8, hipMemcpyHostToDevice, s));
  k_sel_count<<<nb, ST, 0, s>>>(tab, rep, n, keep, tile_cnt, tile_by);
  rk::k_csv_scan<uint64_t><<<1, 1024, 0, s>>>(tile_cnt, nb, tile_off);
  k_sel_bases<<<(ns + 1 + WAVES - 1) / WAVES + 1, ST, 0, s>>>(tab, rep, keep, tile_off, tile_by,
                                                              nb, base, by);
  k_sel_scatter<<<nb, ST, 0, s>>>(tab, Res3{order, gid, rep}, n, keep, tile_off, base,
                                  Out3{o_order, o_gid, o_rep});
  HIPCHK(ctx, hipMemcpyAsync(hdown.data(), down, hdown.size() * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipEventRecord(ctx->ev1, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  HIPCHK(ctx, hipGetLastError());
  float ms = 0;
  HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  for (uint32_t k = 0; k < ns; ++k) {
    kept[k] = hdown[k + 1] - hdown[k];
    if (hdown[k + 1] < hdown[k] || kept[k] > n_out[k]) {
      ctx->err = "select: a set's kept count exceeds its rows";
      return RK_E_INTERNAL;
    }
  }
  put_stats(ctx, ns, n_out, kept, &hdown[ns + 1], ms);
  return RK_OK;
}

extern "C" int rk_result_select(rk_ctx *ctx, const rk_result *res, uint32_t keep, uint32_t flags,
                                rk_result *out) {
  if (!res || !out || !valid_keep(keep) || (flags & ~(uint32_t)RK_RES_DEVICE)) return RK_E_ARG;
  if ((flags & RK_RES_DEVICE) && !ctx) return RK_E_ARG;
  const uint64_t n = res->n_out;
  if (n && (!res->out_order || !res->gid || !res->repval || !out->out_order || !out->gid ||
            !out->repval))
    return RK_E_ARG;
  if (n && (out->out_order == res->out_order || out->gid == res->gid ||
            out->repval == res->repval))
    return RK_E_ARG;
  if (ctx) ctx->err.clear();
  return guarded(ctx, [&]() -> int {
    const uint64_t off[2] = {0, n};
    uint64_t kept = 0;
    const int rc = select_any(ctx, 1, off, &n, res->out_order, res->gid, res->repval, keep, flags,
                              out->out_order, out->gid, out->repval, &kept);
    if (rc) return rc;
    out->n_out = kept;
    out->n_groups = res->n_groups;
    return RK_OK;
  });
}

extern "C" int rk_batch_result_select(rk_ctx *ctx, uint32_t nsets, const uint64_t *set_off,
                                      const rk_batch_result *res, uint32_t keep, uint32_t flags,
                                      rk_batch_result *out) {
  if (!valid_keep(keep) || (flags & ~(uint32_t)RK_RES_DEVICE)) return RK_E_ARG;
  if ((flags & RK_RES_DEVICE) && !ctx) return RK_E_ARG;
  if (nsets == 0) return RK_OK;
  if (!set_off || !res || !out || !res->n_out || !out->n_out) return RK_E_ARG;
  if (check_table(nsets, set_off, res->n_out)) return RK_E_ARG;
  uint64_t rows = 0;
  for (uint32_t k = 0; k < nsets; ++k) rows += res->n_out[k];
  if (rows && (!res->out_order || !res->gid || !res->repval || !out->out_order || !out->gid ||
               !out->repval))
    return RK_E_ARG;
  if (rows && (out->out_order == res->out_order || out->gid == res->gid ||
               out->repval == res->repval))
    return RK_E_ARG;
  if (out->n_out == res->n_out) return RK_E_ARG;
  if (ctx) ctx->err.clear();
  return guarded(ctx, [&]() -> int {
    const int rc = select_any(ctx, nsets, set_off, res->n_out, res->out_order, res->gid,
                              res->repval, keep, flags, out->out_order, out->gid, out->repval,
                              out->n_out);
    if (rc) return rc;
    if (res->n_groups && out->n_groups && res->n_groups != out->n_groups)
      std::copy(res->n_groups, res->n_groups + nsets, out->n_groups);
    return RK_OK;
  });
}

extern "C" int rk_get_select_stats(const rk_ctx *ctx, rk_select_stats *st) {
  if (!ctx || !st) return RK_E_ARG;
  *st = ctx->select;
  return RK_OK;
}

extern "C" uint32_t rk_select_tile(void) { return T; }

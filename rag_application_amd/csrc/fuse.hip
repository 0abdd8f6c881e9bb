// N-way fusion of ranked lists (hx_fuse; include/hx.h states the arithmetic, DESIGN.md section 30 the kernel): reciprocal
// rank fusion with weights, or distribution-based score fusion (every list normalised to its mean +- 3 standard
// deviations), over up to 8 lists and 4096 slots per query.  One workgroup per query, everything in LDS:
//   slots   the live entries of the lists, list after list: slot = off_l + rank (off_l = the entries of the lists before l);
//   stats   (DBSF) the fixed-tree sums of hx.h over the slots of every list at once, in fp64, in place;
//   contrib c_l(r) of every slot, fp32;
//   tags    one 64-bit word per slot, sorted descending: live bit | ~id | 7 - list | 4095 - slot, so that the entries of an
//           id are one run in ascending (list, rank) order.  The head of a run adds the contribution of the first entry of
//           every list in it, in list order -- no entry searches another list (k_rrf does, quadratic in the length);
//   fused   make_key(fused score, id) at the heads, 0 elsewhere, over the tags; sorted descending; the first `limit` leave.
// LDS of the general form: 4096 x 8 B (stats, then tags, then fused keys) + 4096 x 4 B (contributions) = 48 KB.
#include "hx_common.hpp"
#include "kernels.hpp"
#include "wsort.hpp"
#include "../../include/hx.h"

namespace hx {

// IEEE fp32 1/x through fp64 (innocuous double rounding): select.hip, k_rrf
__device__ __forceinline__ float fuse_rcp_f32_rn(float x) { return (float)__ddiv_rn(1.0, (double)x); }

// Descending sort of buf[0, P) by a workgroup of NT threads; P = 64 E * 2^m <= NT * E, block-uniform; buf is complete and
// a barrier has passed.  Wave w sorts the run [64 E w, 64 E (w + 1)) in registers (wsort.hpp) and stores it -- an odd run
// reversed -- which is the state of the bitonic network after its stage k = 64 E.  Of a later stage k the strides j >= 64 E
// run over LDS, one barrier each; below them every run is a bitonic sequence of its own, merged in registers (a run that
// the network wants ascending is read and written back to front).  On return buf is sorted and a barrier has passed.
template <int NT, int E>
__device__ __forceinline__ void block_sort_desc(uint64_t* buf, int P, int tid) {
  constexpr int R = 64 * E;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool on = w * R < P;
  uint64_t v[E];
  if (on) {
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = buf[w * R + e * 64 + lane];   // (the order inside an unsorted run is free)
    w_sort<R>(v, lane);
    const bool rev = (w & 1) != 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int j = lane * E + e;
      buf[w * R + (rev ? R - 1 - j : j)] = v[e];
    }
  }
  __syncthreads();
  for (int k = 2 * R; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= R; j >>= 1) {
      for (int p = tid; p < (P >> 1); p += NT) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const uint64_t x = buf[i], y = buf[i | j];
        const bool desc = (i & k) == 0;
        if (desc ? (x < y) : (x > y)) {
          buf[i] = y;
          buf[i | j] = x;
        }
      }
      __syncthreads();
    }
    if (on) {
      const bool rev = ((w * R) & k) != 0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int j = lane * E + e;
        v[e] = buf[w * R + (rev ? R - 1 - j : j)];
      }
      w_merge<R, R / 2>(v, lane);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int j = lane * E + e;
        buf[w * R + (rev ? R - 1 - j : j)] = v[e];
      }
    }
    __syncthreads();
  }
}

// T(v) of hx.h for every list at once, in place: slot s = off_l + r holds v_l[r]; afterwards slot off_l holds T(v_l).  A
// level h touches the lists with h < n_l (h is a power of two: h < n_l is h < P_l); padding reads as +0.0.
template <int NT, int E>
__device__ __forceinline__ void tree_sums(double* d, const int (&lst)[E], const int (&rnk)[E], const int* s_n, int total,
                                          int hmax, int tid) {
  for (int h = hmax; h >= 1; h >>= 1) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int s = tid + e * NT;
      if (s < total) {
        const int n = s_n[lst[e]], r = rnk[e];
        if (r < h && h < n) d[s] = __dadd_rn(d[s], r + h < n ? d[s + h] : 0.0);
      }
    }
    __syncthreads();
  }
}

template <int NT, int E>
__global__ __launch_bounds__(NT) void k_fuse(FuseArgs a) {
  constexpr int CAP = NT * E;
  static_assert(CAP <= 4096, "a tag holds 12 bits of slot");
  __shared__ __attribute__((aligned(16))) uint64_t buf[CAP];     // fp64 statistics, then tags, then fused keys
  __shared__ float contrib[CAP];
  __shared__ int s_n[FUSE_MAX_LISTS], s_off[FUSE_MAX_LISTS + 1];
  __shared__ double s_mean[FUSE_MAX_LISTS], s_lo[FUSE_MAX_LISTS], s_den[FUSE_MAX_LISTS];
  __shared__ int s_flat[FUSE_MAX_LISTS];                         // DBSF: the list's normalised scores are all 0.5
  __shared__ int s_heads;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nl = a.n_lists;
  if (tid < nl) {
    int n = a.cnt[tid][b];
    n = n < 0 ? 0 : (n < a.stride[tid] ? n : a.stride[tid]);
    s_n[tid] = n;
  }
  if (tid == 0) s_heads = 0;
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int l = 0; l < nl; ++l) {
      s_off[l] = o;
      o += s_n[l];
    }
    for (int l = nl; l <= FUSE_MAX_LISTS; ++l) s_off[l] = o;
  }
  __syncthreads();
  const int total = s_off[FUSE_MAX_LISTS];                       // <= the sum of the strides <= CAP (launch_fuse)
  int P = 64 * E;
  while (P < total) P <<= 1;
  int nmax = 0;
  for (int l = 0; l < nl; ++l) nmax = s_n[l] > nmax ? s_n[l] : nmax;
  int hmax = 0;                                                  // the largest power of two below nmax
  for (int h = 1; h < nmax; h <<= 1) hmax = h;

  // the entries of this thread: slots tid + e * NT
  int lst[E], rnk[E];
  uint32_t id[E];
  float sc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int s = tid + e * NT;
    lst[e] = 0;
    rnk[e] = 0;
    id[e] = 0u;
    sc[e] = 0.0f;
    if (s < total) {
      int l = 0;
      for (int x = 1; x < nl; ++x) l += s >= s_off[x] ? 1 : 0;
      const int r = s - s_off[l];
      const uint64_t key = a.keys[l][(int64_t)b * a.stride[l] + r];
      lst[e] = l;
      rnk[e] = r;
      id[e] = key_id(key);
      sc[e] = key_score(key);
    }
  }

  if (a.method == HX_FUSE_DBSF) {
    double* d = (double*)buf;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int s = tid + e * NT;
      if (s < total) d[s] = (double)sc[e];
    }
    __syncthreads();
    tree_sums<NT, E>(d, lst, rnk, s_n, total, hmax, tid);
    if (tid < nl && s_n[tid] > 0) s_mean[tid] = __ddiv_rn(d[s_off[tid]], (double)s_n[tid]);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int s = tid + e * NT;
      if (s < total) {
        const double x = __dsub_rn((double)sc[e], s_mean[lst[e]]);
        d[s] = __dmul_rn(x, x);
      }
    }
    __syncthreads();
    tree_sums<NT, E>(d, lst, rnk, s_n, total, hmax, tid);
    if (tid < nl) {
      const int n = s_n[tid];
      bool flat = true;
      if (n > 1) {
        const double sd = __dsqrt_rn(__ddiv_rn(d[s_off[tid]], (double)(n - 1)));
        if (sd > 0.0) {
          flat = false;
          s_lo[tid] = __dsub_rn(s_mean[tid], __dmul_rn(3.0, sd));
          s_den[tid] = __dmul_rn(6.0, sd);
        }
      }
      s_flat[tid] = flat ? 1 : 0;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int s = tid + e * NT;
      if (s < total) {
        const int l = lst[e];
        const float norm =
            s_flat[l] ? 0.5f : __double2float_rn(__ddiv_rn(__dsub_rn((double)sc[e], s_lo[l]), s_den[l]));
        contrib[s] = __fmul_rn(a.w[l], norm);
      }
    }
    __syncthreads();                                             // the statistics are read: the tags may take their place
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int s = tid + e * NT;
      if (s < total)
        contrib[s] = __fmul_rn(a.w[lst[e]], fuse_rcp_f32_rn(__fadd_rn((float)(rnk[e] + a.rank_base), a.k)));
    }
  }

  // tags, sorted
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int s = tid + e * NT;
    if (s < P)
      buf[s] = s < total ? (1ull << 63) | ((uint64_t)(~id[e]) << 15) | ((uint64_t)(7 - lst[e]) << 12) | (uint64_t)(4095 - s)
                         : 0ull;
  }
  __syncthreads();
  block_sort_desc<NT, E>(buf, P, tid);

  // the head of every run of one id adds the run's contributions: the first entry of each list, lists ascending
  uint64_t fk[E];
  int heads = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = tid + e * NT;
    fk[e] = 0ull;
    if (i < total) {
      const uint64_t t = buf[i];
      const uint32_t nid = (uint32_t)(t >> 15);                  // ~id
      if (i == 0 || (uint32_t)(buf[i - 1] >> 15) != nid) {
        float f = 0.0f;
        int prev = -1;
        for (int j = i; j < total; ++j) {
          const uint64_t u = buf[j];
          if ((uint32_t)(u >> 15) != nid) break;
          const int l = 7 - (int)((u >> 12) & 7u);
          if (l != prev) f = __fadd_rn(f, contrib[4095 - (int)(u & 4095u)]);
          prev = l;
        }
        fk[e] = make_key(f, ~nid);
        ++heads;
      }
    }
  }
  if (heads) atomicAdd(&s_heads, heads);
  __syncthreads();                                               // every tag is read: the fused keys take their place
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = tid + e * NT;
    if (i < P) buf[i] = fk[e];
  }
  __syncthreads();
  block_sort_desc<NT, E>(buf, P, tid);

  const int m = s_heads < a.limit ? s_heads : a.limit;
  uint64_t* o = a.out + (int64_t)b * a.limit;
  for (int t = tid; t < a.limit; t += NT) o[t] = t < m ? buf[t] : 0ull;
  if (tid == 0) a.out_cnt[b] = m;
}

int fuse_form(int total_slots) { return total_slots <= FUSE_SMALL_SLOTS ? 0 : 1; }

void launch_fuse(const FuseArgs& a, int B, hipStream_t st) {
  if (B <= 0) return;
  int total = 0;
  HX_CHECK(a.n_lists >= 1 && a.n_lists <= FUSE_MAX_LISTS, "fuse: n_lists out of range [1, 8]");
  for (int l = 0; l < a.n_lists; ++l) {
    HX_CHECK(a.stride[l] >= 1 && a.stride[l] <= MAX_LIMIT, "fuse: stride out of range [1, 2048]");
    total += a.stride[l];
  }
  HX_CHECK(total <= FUSE_MAX_SLOTS, "fuse: the strides sum above 4096");
  HX_CHECK(a.limit >= 1 && a.limit <= MAX_LIMIT, "fuse: limit out of range [1, 2048]");
  if (fuse_form(total) == 0) hipLaunchKernelGGL((k_fuse<64, 4>), dim3(B), dim3(64), 0, st, a);
  else hipLaunchKernelGGL((k_fuse<512, 8>), dim3(B), dim3(512), 0, st, a);
  HX_HIP(hipGetLastError());
}

}  // namespace hx

// Late-interaction rerank (hx_maxsim): MaxSim of a query's tokens against the stored tokens of every
// row of a ranked pool.  hx.h states the score: I_ij = the int32 dot product of query token i and row token j (int8 MFMA,
// exact), m_i = max_j (float)I_ij * sd_j, t_i = m_i * sq_i, the 64 slots t_0 .. t_63 (+0.0f past Tq) summed by the balanced
// pairwise tree in index order, + 0.0f.  Every product and sum is a single fp32 operation (-ffp-contract=off and the _rn
// intrinsics).
#include <mutex>
#include "hx_common.hpp"
#include "kernels.hpp"

namespace hx {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int MS_NT = 256;                       // threads of a workgroup: four waves
constexpr int MS_CPB = 16;                       // pool positions of a workgroup, four per wave
constexpr int MS_MT = 4;                         // 16-token tiles of a query (HX_MAXSIM_MAX_QTOKENS = 64)
constexpr uint32_t MS_NULL = 0xFFFFFFFEu;        // HX_PAY_U32_NULL: heads from here on hold no tokens

// One workgroup per (16 pool positions, query); wave w takes the positions c0 + w, c0 + w + 4, ...  The operand maps are
// scan8.hip's: lane = 16 hh + r holds bytes [16 hh, 16 hh + 16) of the 64-byte k-step of token r of its tile, for both
// operands; the C tile holds query token 4 hh + e (register e) against row token r.
//  KS > 0  dim_t = 64 KS <= 128: the wave holds the query's fragments in registers, read once from global memory;
//  KS = 0  wider tokens: the workgroup stages the fragments in LDS, in fragment order (one 1 KB block per (tile, k-step):
//          a wave's read of a block is conflict-free), and every MFMA reads its query operand from there.
// The row's tokens are read straight from the column, 16 tokens per tile, one 16-byte load per lane and k-step.  A tile's
// columns past Td read token Td - 1 (an address inside the row) and enter the max as -inf; query rows past Tq never reach
// the MFMA's result: their slots are +0.0f.
template <int KS>
__global__ __launch_bounds__(MS_NT) __attribute__((amdgpu_waves_per_eu(4))) void k_maxsim_score(MaxsimArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ms_smem[];
  i32x4* qs = (i32x4*)ms_smem;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, r = lane & 15, hh = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t q0 = a.q_indptr[b];
  const int tq = (int)(a.q_indptr[b + 1] - q0);  // 1 .. 64 (checked on the host)
  const int mtq = (tq + 15) >> 4;
  const int ksd = a.dim_t >> 6;
  const uint8_t* qb = (const uint8_t*)a.q8 + q0 * a.dim_t;
  i32x4 qf[MS_MT][KS > 0 ? KS : 1];
  if constexpr (KS > 0) {
#pragma unroll
    for (int mt = 0; mt < MS_MT; ++mt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int i = mt * 16 + r;
        qf[mt][ks] = i < tq ? *(const i32x4*)(qb + (int64_t)i * a.dim_t + ks * 64 + hh * 16) : i32x4{0, 0, 0, 0};
      }
  } else {
    const int cpt = a.dim_t >> 4;                // 16-byte chunks of a token
    for (int x = tid; x < mtq * 16 * cpt; x += MS_NT) {
      const int i = x / cpt, cb = x - i * cpt;
      const i32x4 v = i < tq ? *(const i32x4*)(qb + (int64_t)i * a.dim_t + cb * 16) : i32x4{0, 0, 0, 0};
      qs[(((i >> 4) * ksd + (cb >> 2)) << 6) + ((cb & 3) << 4) + (i & 15)] = v;
    }
    __syncthreads();
  }
  const uint64_t* ikeys = a.ikeys + (int64_t)b * a.stride;
  uint64_t* okeys = a.pos_keys + (int64_t)b * a.stride;
  int n = a.counts ? a.counts[b] : a.stride;
  n = n < 0 ? 0 : (n < a.stride ? n : a.stride);
  const int c0 = blockIdx.x * MS_CPB;
  const int cend = c0 + MS_CPB < a.stride ? c0 + MS_CPB : a.stride;
  const float ninf = -__builtin_inff();
  for (int c = c0 + w; c < cend; c += MS_NT / 64) {          // wave-uniform
    uint32_t row = 0, td = 0;
    bool on = false;
    if (c < n) {
      const uint64_t k = ikeys[c];
      const uint32_t id = key_id(k);
      row = id - a.id_base;
      on = k != 0ull && id >= a.id_base && (int64_t)row < a.n_rows;
      if (on && a.eligible) on = (a.eligible[row >> 5] >> (row & 31)) & 1u;
      if (on) {
        td = a.head[row];
        on = td < MS_NULL && td >= 1u;
      }
    }
    on = __builtin_amdgcn_readfirstlane((int)on);
    if (!on) {
      if (lane == 0) okeys[c] = 0ull;
      continue;
    }
    const int Td = __builtin_amdgcn_readfirstlane((int)td);
    const uint8_t* base = (const uint8_t*)(a.words + a.off[row]);      // (64-bit word offsets)
    const float* sc = (const float*)(base + (int64_t)Td * a.dim_t);
    float mx[MS_MT][4];
#pragma unroll
    for (int mt = 0; mt < MS_MT; ++mt)
#pragma unroll
      for (int e = 0; e < 4; ++e) mx[mt][e] = ninf;
    for (int t0 = 0; t0 < Td; t0 += 16) {
      const int j = t0 + r;
      const bool valid = j < Td;
      const int jj = valid ? j : Td - 1;
      const uint8_t* p = base + (int64_t)jj * a.dim_t + hh * 16;
      const float sd = sc[jj];
      i32x4 acc[MS_MT];
#pragma unroll
      for (int mt = 0; mt < MS_MT; ++mt) acc[mt] = i32x4{0, 0, 0, 0};
      if constexpr (KS > 0) {
        i32x4 d[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) d[ks] = *(const i32x4*)(p + ks * 64);
#pragma unroll
        for (int mt = 0; mt < MS_MT; ++mt) {
          if (mt < mtq) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc[mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(qf[mt][ks], d[ks], acc[mt], 0, 0, 0);
          }
        }
      } else {
        for (int ks = 0; ks < ksd; ++ks) {
          const i32x4 d = *(const i32x4*)(p + ks * 64);
#pragma unroll
          for (int mt = 0; mt < MS_MT; ++mt) {
            if (mt < mtq) acc[mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(qs[((mt * ksd + ks) << 6) + lane], d, acc[mt], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int mt = 0; mt < MS_MT; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = valid ? __fmul_rn((float)acc[mt][e], sd) : ninf;
          mx[mt][e] = v > mx[mt][e] ? v : mx[mt][e];
        }
    }
    // m_i: the max over the 16 lanes that hold query token i; t_i; the tree
    float tile[MS_MT];
#pragma unroll
    for (int mt = 0; mt < MS_MT; ++mt) {
      float t[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float m = mx[mt][e];
#pragma unroll
        for (int o = 1; o <= 8; o <<= 1) {
          const float y = __shfl_xor(m, o, 64);
          m = y > m ? y : m;
        }
        const int i = mt * 16 + hh * 4 + e;                  // (the scale: one cached load per candidate, not 16 registers)
        t[e] = i < tq ? __fmul_rn(m, a.qscale[q0 + i]) : 0.0f;
      }
      float s = __fadd_rn(__fadd_rn(t[0], t[1]), __fadd_rn(t[2], t[3]));
      s = __fadd_rn(s, __shfl_xor(s, 16, 64));
      s = __fadd_rn(s, __shfl_xor(s, 32, 64));
      tile[mt] = s;
    }
    float score = __fadd_rn(__fadd_rn(tile[0], tile[1]), __fadd_rn(tile[2], tile[3]));
    score = __fadd_rn(score, 0.0f);
    if (lane == 0) okeys[c] = ((uint64_t)f32_orderable(score) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)c);
  }
}

// sorted position keys -> the keys of the result, in place
__global__ __launch_bounds__(256) void k_maxsim_finish(const uint64_t* __restrict__ keys, int stride, uint64_t* sorted,
                                                        float* first, int B, int limit) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= (int64_t)B * limit) return;
  const int b = (int)(x / limit);
  const uint64_t k = sorted[x];
  float f = -__builtin_inff();
  if (k != 0ull) {
    const uint32_t pos = 0xFFFFFFFFu - (uint32_t)k;
    const uint64_t src = keys[(int64_t)b * stride + pos];
    sorted[x] = (k & 0xFFFFFFFF00000000ull) | (src & 0xFFFFFFFFull);
    f = key_score(src);
  }
  if (first) first[x] = f;
}

template <int KS>
static void maxsim_launch(const MaxsimArgs& a, int B, size_t lds, hipStream_t st) {
  if (lds > 32768) {   // the dynamic-LDS opt-in is a property of the function ON A DEVICE: once per device, under a lock
    static std::mutex mu;
    static bool attr_set[64] = {};
    int dev = 0;
    HX_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
      HX_HIP(hipFuncSetAttribute((const void*)k_maxsim_score<KS>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
      if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
  }
  hipLaunchKernelGGL(k_maxsim_score<KS>, dim3((a.stride + MS_CPB - 1) / MS_CPB, B), dim3(MS_NT), lds, st, a);
  HX_HIP(hipGetLastError());
}

void launch_maxsim_score(const MaxsimArgs& a, int B, hipStream_t st) {
  switch (a.dim_t / 64) {
    case 1: maxsim_launch<1>(a, B, 0, st); break;
    case 2: maxsim_launch<2>(a, B, 0, st); break;   // (three k-steps in registers would spill at four waves per SIMD)
    default: maxsim_launch<0>(a, B, (size_t)MS_MT * (a.dim_t / 64) * 1024, st); break;   // at most 64 KB
  }
}

void launch_maxsim_finish(const uint64_t* keys, int stride, uint64_t* sorted, float* first, int B, int limit, hipStream_t st) {
  const int64_t n = (int64_t)B * limit;
  hipLaunchKernelGGL(k_maxsim_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, stride, sorted, first, B, limit);
  HX_HIP(hipGetLastError());
}

}  // namespace hx

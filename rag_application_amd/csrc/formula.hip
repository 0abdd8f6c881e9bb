// Score-boosting search (hx_formula): every position of a ranked pool is valued by a postfix
// program over an fp64 stack -- the pool key's score, cells of F64 payload columns, bits of condition planes, constants --
// and the pool is ranked again by that value.  Every operation is ONE IEEE double operation, round to nearest, never fused
// (-ffp-contract=off and the _rn intrinsics), and the exponential is the project's own (hx_exp, stated in hx.h), so a numpy
// float64 restatement gives the same bits.  The value of a position is the stack's last entry as fp32, + 0.0f.
#include "index.hpp"
#include "wsort.hpp"

namespace hx {

constexpr int F_NT = 256;                         // threads of the workgroup
constexpr int F_RUN = 512;                        // keys one wave sorts in registers (E = 8)
constexpr int F_POOL = MAX_LIMIT;                 // most keys of a pool
static_assert(FORMULA_MAX_OPS == HX_FORMULA_MAX_OPS && FORMULA_MAX_PLANES == HX_FORMULA_MAX_PLANES &&
              FORMULA_MAX_COLS == HX_PAY_MAX_COLUMNS && F_POOL == 4 * F_RUN, "kernels.hpp and hx.h disagree");

// hx.h states it; k in [-1021, 1023] and p in [0.70, 1.42], so ldexp never hands out a subnormal
__device__ __forceinline__ double hx_exp(double x) {
  if (x != x) return x;
  if (x > 709.0) return __builtin_inf();
  if (x < -708.0) return 0.0;
  const double k = __builtin_rint(__dmul_rn(x, 1.4426950408889634));
  const double r = __dsub_rn(__dsub_rn(x, __dmul_rn(k, 6.93147180369123816490e-01)),
                             __dmul_rn(k, 1.90821492927058770002e-10));
  constexpr double c[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0,
                            1.0 / 40320.0, 1.0 / 362880.0, 1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0,
                            1.0 / 6227020800.0};
  double p = c[13];
#pragma unroll
  for (int i = 12; i >= 0; --i) p = __dadd_rn(__dmul_rn(p, r), c[i]);
  return __builtin_ldexp(p, (int)k);
}

__device__ __forceinline__ double f_abs(double x) { return __builtin_fabs(x); }

// One workgroup of 256 threads per query.
//  value  the program and its immediates go from the kernel arguments to LDS; thread t values the positions t + 256 k.
//         A position is eligible by hx_mmr's rule.  The stack is `top` (a register) over stk[depth][thread] in LDS: a
//         dynamically indexed private array would live in scratch; the column [.][t] is thread t's alone, and 64
//         consecutive doubles of one depth are conflict-free.  The program is straight-line, so the depth is uniform.
//         key = orderable(value) << 32 | 0xFFFFFFFF - position, 0 for a position that is not eligible, was dropped (its
//         value is not finite: counted) or lies under the threshold;
//  sort   P = 512, 1024 or 2048 slots >= the pool.  Wave w sorts the run [512 w, 512 w + 512) in registers (wsort.hpp),
//         descending, and stores it -- an odd run reversed -- so that the runs are the input of the bitonic network's stage
//         k = 1024; the stages k = 1024, 2048 run over LDS;
//  out    slot t < min(survivors, limit): make_key(value, the id of keys[position]), the position and (out_base != NULL)
//         the score keys[position] carried; (0, -1, -inf) past them.
__global__ __launch_bounds__(F_NT) void k_formula(FormulaArgs a) {
  __shared__ double stk[HX_FORMULA_MAX_STACK][F_NT];                   // 32 KB
  __shared__ __attribute__((aligned(16))) uint64_t skey[F_POOL];       // 16 KB
  __shared__ uint64_t imm[HX_FORMULA_MAX_OPS];                         // 2 KB
  __shared__ uint8_t opc[HX_FORMULA_MAX_OPS], oarg[HX_FORMULA_MAX_OPS];
  __shared__ int s_cnt, s_drop;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t* keys = a.keys + (int64_t)b * a.stride;      // as the caller gave them: what the result carries
  const uint64_t* ikeys = a.ikeys + (int64_t)b * a.stride;    // the same slots with internal ids: what names the rows
  int n = a.counts ? a.counts[b] : a.stride;
  n = n < 0 ? 0 : (n < a.stride ? n : a.stride);
  const int n_ops = a.n_ops;
  for (int i = tid; i < n_ops; i += F_NT) {
    imm[i] = a.imm[i];
    opc[i] = a.op[i];
    oarg[i] = a.arg[i];
  }
  if (tid == 0) {
    s_cnt = 0;
    s_drop = 0;
  }
  const int P = n <= F_RUN ? F_RUN : (n <= 2 * F_RUN ? 2 * F_RUN : 4 * F_RUN);
  __syncthreads();
  int kept = 0, dropped = 0;
  for (int i = tid; i < P; i += F_NT) {
    uint64_t out = 0ull;
    const uint64_t k = i < n ? ikeys[i] : 0ull;
    const uint32_t id = key_id(k), row = id - a.id_base;
    bool on = k != 0ull && id >= a.id_base && (int64_t)row < a.n_rows;
    if (on && a.eligible) on = (a.eligible[row >> 5] >> (row & 31)) & 1u;
    if (on) {
      double top = 0.0;
      int d = 0;                                   // entries of the stack: top and stk[0, d - 1)
      for (int ip = 0; ip < n_ops; ++ip) {
        const int op = opc[ip];
        const uint64_t im = imm[ip];
        if (op <= HX_F_COND) {                     // the pushes
          double x;
          if (op == HX_F_CONST) {
            x = __longlong_as_double((long long)im);
          } else if (op == HX_F_SCORE) {
            x = (double)key_score(k);
          } else if (op == HX_F_VAR) {
            const int c = oarg[ip];
            const uint64_t cell = ((uint64_t)a.col_hi[c][row] << 32) | a.col_lo[c][row];
            x = __longlong_as_double((long long)((cell == HX_PAY_F64_MISSING || cell == HX_PAY_F64_NULL) ? im : cell));
          } else {
            x = ((a.planes[oarg[ip]][row >> 5] >> (row & 31)) & 1u) ? 1.0 : 0.0;
          }
          if (d > 0) stk[d - 1][tid] = top;
          top = x;
          ++d;
        } else if (op == HX_F_ADD || op == HX_F_MUL || op == HX_F_DIV) {
          const double y = top, x = stk[d - 2][tid];
          --d;
          if (op == HX_F_ADD) top = __dadd_rn(x, y);
          else if (op == HX_F_MUL) top = __dmul_rn(x, y);
          else top = y == 0.0 ? __longlong_as_double((long long)im) : __ddiv_rn(x, y);
        } else {
          const double c = __longlong_as_double((long long)im);
          switch (op) {
            case HX_F_NEG: top = -top; break;
            case HX_F_ABS: top = f_abs(top); break;
            case HX_F_SQRT: top = __dsqrt_rn(top); break;
            case HX_F_EXP: top = hx_exp(top); break;
            case HX_F_LIN_DECAY: {
              const double t = __dsub_rn(1.0, __dmul_rn(c, f_abs(top)));
              top = t < 0.0 ? 0.0 : t;             // (a NaN stays a NaN)
              break;
            }
            case HX_F_EXP_DECAY: top = hx_exp(__dmul_rn(c, f_abs(top))); break;
            default: top = hx_exp(__dmul_rn(c, __dmul_rn(top, top))); break;   // HX_F_GAUSS_DECAY
          }
        }
      }
      const float v = __fadd_rn(__double2float_rn(top), 0.0f);
      if (!(__builtin_fabsf(v) < __builtin_inff())) {
        ++dropped;
      } else if (!a.has_threshold || !(v < a.threshold)) {
        out = ((uint64_t)f32_orderable(v) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)i);
        ++kept;
      }
    }
    skey[i] = out;
  }
  if (kept) atomicAdd(&s_cnt, kept);
  if (dropped) atomicAdd(&s_drop, dropped);
  __syncthreads();
  if (w * F_RUN < P) {
    uint64_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = skey[w * F_RUN + e * 64 + lane];   // (the order inside an unsorted run is free)
    w_sort<F_RUN>(v, lane);
    const bool rev = (w & 1) != 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = lane * 8 + e;
      skey[w * F_RUN + (rev ? F_RUN - 1 - j : j)] = v[e];
    }
  }
  __syncthreads();
  for (int k = 2 * F_RUN; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += F_NT) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t x = skey[i], y = skey[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (x < y) : (x > y)) {
            skey[i] = y;
            skey[ixj] = x;
          }
        }
      }
      __syncthreads();
    }
  }
  const int m = s_cnt < a.limit ? s_cnt : a.limit;
  uint64_t* okeys = a.out_keys + (int64_t)b * a.limit;
  int* opos = a.out_pos + (int64_t)b * a.limit;
  float* obase = a.out_base ? a.out_base + (int64_t)b * a.limit : nullptr;
  for (int t = tid; t < a.limit; t += F_NT) {
    uint64_t ok = 0ull;
    int pos = -1;
    float base = -__builtin_inff();
    if (t < m) {
      const uint64_t s = skey[t];
      pos = (int)(0xFFFFFFFFu - (uint32_t)s);
      const uint64_t src = keys[pos];
      ok = make_key(orderable_f32((uint32_t)(s >> 32)), key_id(src));
      base = key_score(src);
    }
    okeys[t] = ok;
    opos[t] = pos;
    if (obase) obase[t] = base;
  }
  if (tid == 0) {
    a.out_counts[b] = m;
    a.out_dropped[b] = s_drop;
  }
}

void launch_formula(const FormulaArgs& a, int B, hipStream_t st) {
  hipLaunchKernelGGL(k_formula, dim3(B), dim3(F_NT), 0, st, a);
  HX_HIP(hipGetLastError());
}

// Every refusal of hx_formula that concerns the program, before any device work, and the program as the kernel takes
// it: one byte of op and of argument per op (a VAR's argument = its entry in the table of distinct columns).
void formula_lower(hx_index* h, const hx_formula_op* ops, int32_t n_ops, int32_t n_planes, FormulaArgs& a) {
  HX_CHECK(ops != nullptr, "NULL argument");
  HX_CHECK(n_ops >= 1 && n_ops <= HX_FORMULA_MAX_OPS, "formula: n_ops out of range [1, 256]");
  HX_CHECK(n_planes >= 0 && n_planes <= HX_FORMULA_MAX_PLANES, "formula: n_planes out of range [0, 8]");
  int depth = 0, n_cols = 0;
  int col_id[HX_PAY_MAX_COLUMNS];
  for (int i = 0; i < n_ops; ++i) {
    const hx_formula_op& o = ops[i];
    int arg = 0;
    switch (o.op) {
      case HX_F_CONST:
      case HX_F_SCORE:
        ++depth;
        break;
      case HX_F_VAR: {
        const hx_index::PayCol& c = pay_col(h, o.arg);
        HX_CHECK(c.kind == HX_PAY_F64, "formula: the column kind of a variable must be HX_PAY_F64");
        HX_CHECK(c.filled == h->n, "formula: the column is not filled to the index's row count (hx_count)");
        double dflt;
        std::memcpy(&dflt, &o.imm, 8);
        HX_CHECK(dflt == dflt, "formula: the default of a variable is NaN");
        for (arg = 0; arg < n_cols && col_id[arg] != o.arg; ++arg) {
        }
        if (arg == n_cols) {
          HX_CHECK(n_cols < HX_PAY_MAX_COLUMNS, "formula: too many columns");
          col_id[n_cols] = o.arg;
          a.col_lo[n_cols] = c.p0;
          a.col_hi[n_cols] = c.p1;
          ++n_cols;
        }
        ++depth;
        break;
      }
      case HX_F_COND:
        HX_CHECK(o.arg >= 0 && o.arg < n_planes, "formula: condition plane index out of range");
        arg = o.arg;
        ++depth;
        break;
      case HX_F_ADD:
      case HX_F_MUL:
      case HX_F_DIV:
        HX_CHECK(depth >= 2, "formula: the program underflows its stack");
        --depth;
        break;
      case HX_F_NEG:
      case HX_F_ABS:
      case HX_F_SQRT:
      case HX_F_EXP:
      case HX_F_LIN_DECAY:
      case HX_F_EXP_DECAY:
      case HX_F_GAUSS_DECAY:
        HX_CHECK(depth >= 1, "formula: the program underflows its stack");
        break;
      default:
        HX_CHECK(false, "formula: unknown op");
    }
    HX_CHECK(depth <= HX_FORMULA_MAX_STACK, "formula: the program passes the stack limit of 16");
    a.op[i] = (uint8_t)o.op;
    a.arg[i] = (uint8_t)arg;
    a.imm[i] = o.imm;
  }
  HX_CHECK(depth == 1, "formula: the program must end with exactly one entry");
  a.n_ops = n_ops;
}

}  // namespace hx

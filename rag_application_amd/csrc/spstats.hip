// Collection term statistics of the sparse stage and the IDF modifier built on them (hx.h states
// the arithmetic): per-term document frequencies read off the inverted index's posting directories, the number of rows
// that hold a sparse vector, and q_t * ln(1 + (N - df + 0.5) / (df + 0.5)) for every query weight.  Everything goes to
// the caller's stream; nothing is read back.
//
// The weights are part of the bit-exact contract: every double operation below is ONE IEEE operation (-ffp-contract=off
// and the _rn intrinsics, as formula.hip), and the logarithm is the project's own (hx_ln), so a numpy model restates it
// without depending on any libm.
#include "index.hpp"
#include "spfind.hpp"

namespace hx {

// df of one position per wave: the term's row of each view's directory
__global__ __launch_bounds__(256) void k_sparse_df(SparseIndexView v0, SparseIndexView v1, const int32_t* q_idx,
                                                   int64_t nnz, int64_t* df) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nnz; i += stride) {   // (wave-uniform)
    const int32_t id = q_idx[i];
    int64_t n = 0;
    if (id >= 0) {
      const uint32_t term = (uint32_t)id;
      if (v0.n_live > 0) {
        const int r = sp_find_term_wave(v0.uterms, v0.n_live, term, lane);
        if (r >= 0) {
          const uint32_t* row = v0.ptr + (int64_t)r * (v0.n_segments + 1);
          n += (int64_t)(row[v0.n_segments] - row[0]);
        }
      }
      if (v1.n_live > 0) {
        const int r = sp_find_term_wave(v1.uterms, v1.n_live, term, lane);
        if (r >= 0) {
          const uint32_t* row = v1.ptr + (int64_t)r * (v1.n_segments + 1);
          n += (int64_t)(row[v1.n_segments] - row[0]);
        }
      }
    }
    if (lane == 0) df[i] = n;
  }
}
void launch_sparse_df(const SparseIndexView* ix, const int32_t* q_idx, int64_t nnz, int64_t* df, hipStream_t st) {
  if (nnz <= 0) return;
  const int64_t blocks = std::min<int64_t>((nnz + 3) / 4, 1 << 16);
  hipLaunchKernelGGL(k_sparse_df, dim3((unsigned)blocks), dim3(256), 0, st, ix[0], ix[1], q_idx, nnz, df);
  HX_HIP(hipGetLastError());
}

// rows with a sparse vector: a ballot per wave and step, one atomic per workgroup
__global__ __launch_bounds__(256) void k_sparse_rows_nonempty(const int64_t* indptr, int64_t rows,
                                                              unsigned long long* n_docs) {
  __shared__ unsigned long long s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  unsigned long long mine = 0;     // the wave's count (the same in every lane)
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < rows; base += stride) {
    const int64_t r = base + threadIdx.x;
    const bool full = r < rows && indptr[r + 1] > indptr[r];
    mine += (unsigned long long)__popcll(__ballot(full));
  }
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_n, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(n_docs, s_n);
}
void launch_sparse_rows_nonempty(const int64_t* indptr, int64_t rows, int64_t* n_docs, hipStream_t st) {
  HX_HIP(hipMemsetAsync(n_docs, 0, 8, st));
  if (rows <= 0) return;
  const int64_t blocks = std::min<int64_t>((rows + 255) / 256, 2048);
  hipLaunchKernelGGL(k_sparse_rows_nonempty, dim3((unsigned)blocks), dim3(256), 0, st, indptr, rows,
                     (unsigned long long*)n_docs);
  HX_HIP(hipGetLastError());
}

// hx_ln (hx.h): the natural logarithm of a positive normal double, 2 atanh((m - 1) / (m + 1)) + e ln 2 with m in
// [sqrt(1/2), sqrt(2)); every operation is one rounding
__device__ __forceinline__ double hx_ln(double x) {
  constexpr double c[12] = {1.0 / 1.0,  1.0 / 3.0,  1.0 / 5.0,  1.0 / 7.0,  1.0 / 9.0,  1.0 / 11.0,
                            1.0 / 13.0, 1.0 / 15.0, 1.0 / 17.0, 1.0 / 19.0, 1.0 / 21.0, 1.0 / 23.0};
  const long long bits = __double_as_longlong(x);
  int e = (int)((bits >> 52) & 0x7FF) - 1022;                                              // frexp: x = m 2^e,
  double m = __longlong_as_double((bits & 0x800FFFFFFFFFFFFFll) | 0x3FE0000000000000ll);   // m in [0.5, 1)
  if (m < 0.7071067811865476) {
    m = __dmul_rn(m, 2.0);
    e -= 1;
  }
  const double s = __ddiv_rn(__dsub_rn(m, 1.0), __dadd_rn(m, 1.0));
  const double z = __dmul_rn(s, s);
  double p = c[11];
#pragma unroll
  for (int i = 10; i >= 0; --i) p = __dadd_rn(__dmul_rn(p, z), c[i]);
  const double t = __dmul_rn(__dmul_rn(2.0, s), p);
  return __dadd_rn(__dmul_rn((double)e, 0.6931471805599453), t);
}

__global__ __launch_bounds__(256) void k_sparse_idf(const float* q_val, const int64_t* df, const int64_t* n_docs,
                                                    int64_t nnz, float* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nnz) return;
  int64_t N = n_docs[0];
  N = N < 0 ? 0 : N;
  int64_t d = df[i];
  d = d < 0 ? 0 : (d > N ? N : d);
  const double num = __dadd_rn(__ll2double_rn(N - d), 0.5);
  const double den = __dadd_rn(__ll2double_rn(d), 0.5);
  const double x = __dadd_rn(1.0, __ddiv_rn(num, den));
  const float idf = __double2float_rn(hx_ln(x));
  out[i] = __fmul_rn(q_val[i], idf);
}
void launch_sparse_idf(const float* q_val, const int64_t* df, const int64_t* n_docs, int64_t nnz, float* out,
                       hipStream_t st) {
  if (nnz <= 0) return;
  hipLaunchKernelGGL(k_sparse_idf, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, q_val, df, n_docs, nnz, out);
  HX_HIP(hipGetLastError());
}

// df of nnz term ids and N, enqueued: the body of hx_sparse_df
static void sparse_df_dev(hx_index* h, const int32_t* q_idx, int64_t nnz, int64_t* df, int64_t* n_docs, hipStream_t st) {
  sparse_up_to_date(h, st);
  SparseIndexView v[2]{};
  const hx_index::SparseIx* ixs[2] = {&h->sp_base, &h->sp_tail};
  for (int k = 0; k < 2; ++k) {
    v[k].ptr = ixs[k]->sp.ptr;
    v[k].uterms = ixs[k]->sp.uterms;
    v[k].n_live = ixs[k]->n_segments ? (int)ixs[k]->sp.n_live : 0;
    v[k].n_segments = ixs[k]->n_segments;
  }
  launch_sparse_df(v, q_idx, nnz, df, st);
  // a row without a sparse vector is an empty document (or, with no posting at all, not in the CSR)
  launch_sparse_rows_nonempty(h->sp_indptr, h->nnz > 0 ? std::min(h->sp_rows, h->n) : 0, n_docs, st);
}

}  // namespace hx

extern "C" {

int hx_sparse_df(hx_index* h, const int32_t* q_idx_dev, int64_t nnz, int64_t* df_dev, int64_t* n_docs_dev,
                 void* stream) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  HX_CHECK(nnz >= 0, "sparse_df: nnz < 0");
  HX_CHECK(n_docs_dev && (nnz == 0 || (q_idx_dev && df_dev)), "sparse_df: NULL argument");
  h->set_device();
  sparse_df_dev(h, q_idx_dev, nnz, df_dev, n_docs_dev, (hipStream_t)stream);
  HX_CATCH
}

int hx_sparse_idf_apply(int32_t device, const float* q_val_dev, const int64_t* df_dev, const int64_t* n_docs_dev,
                        int64_t nnz, float* out_val_dev, void* stream) {
  HX_TRY
  HX_CHECK(nnz >= 0, "sparse_idf_apply: nnz < 0");
  HX_CHECK(n_docs_dev && (nnz == 0 || (q_val_dev && df_dev && out_val_dev)), "sparse_idf_apply: NULL argument");
  HX_HIP(hipSetDevice(device));
  launch_sparse_idf(q_val_dev, df_dev, n_docs_dev, nnz, out_val_dev, (hipStream_t)stream);
  HX_CATCH
}

int hx_sparse_idf_host(hx_index* h, const int32_t* q_idx_host, const float* q_val_host, int64_t nnz,
                       float* out_val_host, int64_t* df_host, int64_t* n_docs_host) {
  HX_TRY
  HX_CHECK(h, "index is NULL");
  HX_CHECK(nnz >= 0, "sparse_idf_host: nnz < 0");
  HX_CHECK(nnz == 0 || (q_idx_host && q_val_host && out_val_host), "sparse_idf_host: NULL argument");
  h->set_device();
  hipStream_t st = nullptr;
  int32_t* idx = (int32_t*)h->ws.get(WS_IDF_IDX, (size_t)std::max<int64_t>(nnz, 1) * 4);
  float* val = (float*)h->ws.get(WS_IDF_VAL, (size_t)std::max<int64_t>(nnz, 1) * 4);
  int64_t* df = (int64_t*)h->ws.get(WS_IDF_DF, (size_t)(nnz + 1) * 8);     // df[nnz] = N
  if (nnz) {
    HX_HIP(hipMemcpyAsync(idx, q_idx_host, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    HX_HIP(hipMemcpyAsync(val, q_val_host, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
  }
  sparse_df_dev(h, idx, nnz, df, df + nnz, st);
  launch_sparse_idf(val, df, df + nnz, nnz, val, st);
  if (nnz) HX_HIP(hipMemcpyAsync(out_val_host, val, (size_t)nnz * 4, hipMemcpyDeviceToHost, st));
  if (nnz && df_host) HX_HIP(hipMemcpyAsync(df_host, df, (size_t)nnz * 8, hipMemcpyDeviceToHost, st));
  if (n_docs_host) HX_HIP(hipMemcpyAsync(n_docs_host, df + nnz, 8, hipMemcpyDeviceToHost, st));
  HX_HIP(hipStreamSynchronize(st));
  HX_CATCH
}

}  // extern "C"

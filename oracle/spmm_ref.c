/* ORACLE (test infrastructure only): plain-C restatement of the CSR SpMM
 * C = A @ B that th.spmm(adj, support) computes (reference layer.py:106).
 * Row by row, nonzeros in CSR order.  The f64 form is the parity checker for
 * large inputs; the f32 form (sequential fp32 accumulation) is a scalar CPU
 * port used for error bounds.  Built by __graft_entry__.build() into
 * oracle/liboracle.so with gcc; never linked into the product. */
#include <stdint.h>
#include <string.h>

void oracle_spmm_csr_f64(const int64_t* rowptr, const int64_t* colind, const double* val, int64_t M,
                         const double* B, int64_t F, double* C) {
  for (int64_t r = 0; r < M; ++r) {
    double* c = C + r * F;
    memset(c, 0, (size_t)F * sizeof(double));
    for (int64_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
      const double a = val[k];
      const double* b = B + colind[k] * F;
      for (int64_t j = 0; j < F; ++j) c[j] += a * b[j];
    }
  }
}

/* The device dropout hash (include/gcnk.h, GCNK_EPI_BIAS_RELU_HASH) written a
 * second time, beside oracle/hash_ref.py: out[i] = h >> 8 for (seed, idx[i]),
 * the 24 bits the uniform (h >> 8) * 2^-24 is made of. */
static uint32_t oracle_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

void oracle_hash_u24(uint64_t seed, const uint64_t* idx, int64_t n, uint32_t* out) {
  const uint32_t seed_lo = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32);
  for (int64_t i = 0; i < n; ++i) {
    uint32_t h = oracle_mix32((uint32_t)idx[i] ^ seed_lo);
    h = oracle_mix32(h ^ (uint32_t)(idx[i] >> 32) ^ seed_hi);
    h = oracle_mix32(h + 0x9e3779b9U);
    out[i] = h >> 8;
  }
}

void oracle_spmm_csr_f32(const int64_t* rowptr, const int64_t* colind, const float* val, int64_t M,
                         const float* B, int64_t F, float* C) {
  for (int64_t r = 0; r < M; ++r) {
    float* c = C + r * F;
    memset(c, 0, (size_t)F * sizeof(float));
    for (int64_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
      const float a = val[k];
      const float* b = B + colind[k] * F;
      for (int64_t j = 0; j < F; ++j) c[j] += a * b[j];
    }
  }
}

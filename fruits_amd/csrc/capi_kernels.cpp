// The thin entries: each checks its arguments and launches one kernel (kernels.h).
#include <mutex>
#include <vector>

#include "capi_common.h"
#include "kernels.h"

using namespace fr::capi;

namespace {
// the grouping tables of RIN / JLD on the host: every entry is checked before a kernel reads
// the device copies
int check_groups(const char *who, const int32_t *h_ndim, int32_t O, const int32_t *h_dims,
                 int32_t J, int64_t D) {
  const std::string w(who);
  if (!h_ndim || !h_dims) return fail(FR_E_ARG, w + ": null host table");
  int64_t total = 0;
  for (int32_t o = 0; o < O; ++o) {
    if (h_ndim[o] < 0) return fail(FR_E_ARG, w + ": negative group size");
    total += h_ndim[o];
  }
  if (total != J) return fail(FR_E_ARG, w + ": the group sizes do not add up to the number of slots");
  for (int32_t j = 0; j < J; ++j)
    if (h_dims[j] < 0 || h_dims[j] >= D)
      return fail(FR_E_DIM, w + ": slot " + std::to_string(j) + " names dimension " +
                                std::to_string(h_dims[j]) + " of " + std::to_string(D));
  return FR_OK;
}
}  // namespace

extern "C" {

int fr_increments(const double *d_X, int64_t rows, int64_t T, int64_t shift, double *d_out,
                  const double *d_head_src, int64_t head, void *stream) {
  if (rows < 0 || T < 0 || shift < 0) return fail(FR_E_ARG, "fr_increments: bad shape");
  if (rows == 0 || T == 0) return FR_OK;
  if (!d_X || !d_out) return fail(FR_E_ARG, "fr_increments: null device pointer");
  hipError_t e = fr::launch_increments(d_X, rows, T, shift, d_out, d_head_src, head,
                                       (hipStream_t)stream);
  return launched(e, "increments launch");
}

int fr_pathlen_lookup(const double *d_X, int64_t N, int64_t D, int64_t T, int32_t norm,
                      int32_t relative, double scale, double *d_out, void *stream) {
  const int exact = (norm & FR_LOOKUP_FAST) ? 0 : 1;
  norm &= ~FR_LOOKUP_FAST;
  if (N < 0 || D < 1 || T < 0 || (norm != 1 && norm != 2))
    return fail(FR_E_ARG, "fr_pathlen_lookup: bad argument");
  if (N == 0 || T == 0) return FR_OK;
  if (!d_X || !d_out) return fail(FR_E_ARG, "fr_pathlen_lookup: null device pointer");
  hipError_t e = fr::launch_pathlen_lookup(d_X, N, D, T, norm, relative, scale, exact, d_out,
                                           (hipStream_t)stream);
  return launched(e, "pathlen_lookup launch");
}

int fr_sieve(int32_t kind, const double *d_A, int64_t N, int64_t T, int64_t a_stride, int32_t inc,
             const int64_t *d_cuts, int64_t cut_rows, int32_t C1, const double *d_q, int32_t Q1,
             double *d_out, int64_t out_stride, void *stream) {
  if (kind < 0 || kind > FR_SIEVE_CUR) return fail(FR_E_ARG, "fr_sieve: unknown kind");
  if (N < 0 || T < 1 || C1 < 2 || (cut_rows != 1 && cut_rows != N))
    return fail(FR_E_ARG, "fr_sieve: bad shape");
  if (kind != FR_SIEVE_END && (Q1 < 2 || !d_q)) return fail(FR_E_ARG, "fr_sieve: bad quantiles");
  if (inc < 0 || inc > 8) return fail(FR_E_LIMIT, "fr_sieve: inc must be in [0, 8]");
  if (N == 0) return FR_OK;
  if (!d_A || !d_cuts || !d_out) return fail(FR_E_ARG, "fr_sieve: null device pointer");
  hipError_t e = fr::launch_sieve(kind, d_A, N, T, a_stride, inc, d_cuts, cut_rows, C1, d_q, Q1,
                                  d_out, out_stride, (hipStream_t)stream);
  return launched(e, "sieve launch");
}

int fr_sieve_implicit(int32_t kind, const double *d_A, int64_t N, int64_t T, int64_t a_stride,
                      const double *d_q, int32_t Q, int32_t segments, double *d_out,
                      int64_t out_stride, void *stream) {
  if (kind != FR_SIEVE_PPV && kind != FR_SIEVE_CPV)
    return fail(FR_E_ARG, "fr_sieve_implicit: unknown kind");
  if (N < 0 || T < 1 || N > 0x7fffffffLL) return fail(FR_E_ARG, "fr_sieve_implicit: bad shape");
  if (Q < 1 || (segments && Q < 2) || !d_q)
    return fail(FR_E_ARG, "fr_sieve_implicit: bad quantiles");
  if (Q - (segments ? 1 : 0) > fr::kImplicitMaxFeatures)
    return fail(FR_E_LIMIT, "fr_sieve_implicit: at most 256 features per sieve");
  if (N == 0) return FR_OK;
  if (!d_A || !d_out) return fail(FR_E_ARG, "fr_sieve_implicit: null device pointer");
  hipError_t e = fr::launch_sieve_implicit(kind, d_A, N, T, a_stride, nullptr, d_q, Q, segments ? 1 : 0,
                                           d_out, out_stride, (hipStream_t)stream);
  return launched(e, "implicit sieve launch");
}

int fr_sieve_implicit_lengths(int32_t kind, const double *d_A, int64_t N, int64_t T, int64_t a_stride,
                              const int32_t *d_lengths, const double *d_q, int32_t Q, int32_t segments,
                              double *d_out, int64_t out_stride, void *stream) {
  if (kind != FR_SIEVE_PPV && kind != FR_SIEVE_CPV)
    return fail(FR_E_ARG, "fr_sieve_implicit_lengths: unknown kind");
  if (N < 0 || T < 1 || N > 0x7fffffffLL || T > 0x7fffffffLL)
    return fail(FR_E_ARG, "fr_sieve_implicit_lengths: bad shape");
  if (Q < 1 || (segments && Q < 2) || !d_q)
    return fail(FR_E_ARG, "fr_sieve_implicit_lengths: bad quantiles");
  if (Q - (segments ? 1 : 0) > fr::kImplicitMaxFeatures)
    return fail(FR_E_LIMIT, "fr_sieve_implicit_lengths: at most 256 features per sieve");
  if (N == 0) return FR_OK;
  if (!d_A || !d_out || !d_lengths) return fail(FR_E_ARG, "fr_sieve_implicit_lengths: null device pointer");
  hipError_t e = fr::launch_sieve_implicit(kind, d_A, N, T, a_stride, d_lengths, d_q, Q, segments ? 1 : 0,
                                           d_out, out_stride, (hipStream_t)stream);
  return launched(e, "implicit sieve launch");
}

int fr_pre_transform(const double *d_A, int64_t N, int64_t T, int64_t a_stride, int32_t inc,
                     double *d_out, void *stream) {
  if (N < 0 || T < 0 || inc < 0 || inc > 8) return fail(FR_E_ARG, "fr_pre_transform: bad argument");
  if (N == 0 || T == 0) return FR_OK;
  if (!d_A || !d_out) return fail(FR_E_ARG, "fr_pre_transform: null device pointer");
  hipError_t e = fr::launch_pre_transform(d_A, N, T, a_stride, inc, d_out, (hipStream_t)stream);
  return launched(e, "pre_transform launch");
}

int fr_standardize(const double *d_X, int64_t rows, int64_t T, int32_t div_std, double eps,
                   double *d_out, void *stream) {
  if (rows < 0 || T < 0) return fail(FR_E_ARG, "fr_standardize: bad shape");
  if (rows == 0 || T == 0) return FR_OK;
  if (!d_X || !d_out) return fail(FR_E_ARG, "fr_standardize: null device pointer");
  hipError_t e = fr::launch_standardize(d_X, rows, T, nullptr, 1, div_std, eps, d_out, (hipStream_t)stream);
  return launched(e, "standardize launch");
}

int fr_standardize_lengths(const double *d_X, int64_t N, int64_t D, int64_t T, const int32_t *d_lengths,
                           int32_t div_std, double eps, double *d_out, void *stream) {
  if (N < 0 || D < 1 || T < 1 || T > 0x7fffffffLL || N * D > 0x7fffffffLL)
    return fail(FR_E_ARG, "fr_standardize_lengths: bad shape");
  if (N == 0) return FR_OK;
  if (!d_X || !d_out || !d_lengths) return fail(FR_E_ARG, "fr_standardize_lengths: null device pointer");
  hipError_t e = fr::launch_standardize(d_X, N * D, T, d_lengths, D, div_std, eps, d_out, (hipStream_t)stream);
  return launched(e, "standardize launch");
}

int fr_coswiss_set_dropout(fr_plan_t *plan, const int32_t *h_indices, int32_t Lmax, int32_t rate,
                           int64_t T) {
  if (!plan || !plan->p || !plan->p->cos || Lmax < 0 || rate < 0 || T < 1 ||
      (rate > 0 && Lmax > 0 && !h_indices))
    return fail(FR_E_ARG, "fr_coswiss_set_dropout: bad argument");
  fr::Plan &p = *plan->p;
  fr::CosProgram &c = *p.cos;
  std::lock_guard<std::mutex> lock(p.mu);
  if (c.d_mask) (void)hipFree(c.d_mask);
  c.d_mask = nullptr;
  c.Lmax = 0;
  c.mask_T = 0;
  if (Lmax == 0) return FR_OK;   // dropout off
  if (Lmax < p.levels)
    return fail(FR_E_ARG, "fr_coswiss_set_dropout: Lmax is shorter than the longest word");
  const size_t rows = (size_t)c.W * c.F * Lmax;
  std::vector<double> mask(rows * (size_t)T, 1.0);
  for (size_t r = 0; r < rows; ++r)
    for (int i = 0; i < rate; ++i) {
      const int32_t idx = h_indices[r * rate + i];
      if (idx < 0 || idx >= T)
        return fail(FR_E_INDEX, "fr_coswiss_set_dropout: index " + std::to_string(idx) +
                                    " is out of bounds for series of length " + std::to_string(T));
      mask[r * (size_t)T + idx] = 0.0;
    }
  int rc = claim_device(p, "fr_coswiss_set_dropout");
  if (rc != FR_OK) return rc;
  HIP_TRY(hipMalloc(&c.d_mask, mask.size() * 8));
  hipError_t e = hipMemcpy(c.d_mask, mask.data(), mask.size() * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(c.d_mask);
    c.d_mask = nullptr;
    return hip_fail(e, "hipMemcpy(dropout mask)");
  }
  c.Lmax = Lmax;
  c.mask_T = T;
  return FR_OK;
}

int fr_coswiss_set_input_stride(fr_plan_t *plan, int64_t unit_stride) {
  if (!plan || !plan->p || !plan->p->cos || unit_stride < 0)
    return fail(FR_E_ARG, "fr_coswiss_set_input_stride: bad argument");
  plan->p->cos->x_unit_stride = unit_stride;
  return FR_OK;
}

int fr_coswiss_ffn(const double *d_X, int64_t N, int64_t D, int64_t T, const double *d_A,
                   const double *d_b, const double *d_C, int32_t hidden, double *d_Z,
                   void *stream) {
  if (N < 0 || D < 1 || T < 0 || hidden < 1) return fail(FR_E_ARG, "fr_coswiss_ffn: bad shape");
  if (N == 0 || T == 0) return FR_OK;
  if (!d_X || !d_A || !d_b || !d_C || !d_Z)
    return fail(FR_E_ARG, "fr_coswiss_ffn: null device pointer");
  hipError_t e = fr::launch_coswiss_ffn(d_X, N, D, T, d_A, d_b, d_C, hidden, d_Z,
                                        (hipStream_t)stream);
  return launched(e, "coswiss ffn launch", "fr_coswiss_ffn: at most 64 hidden units and 16 input dimensions");
}

int fr_arctic_argmax(const double *d_V, int64_t rows, int64_t N, int64_t T, int32_t n_jobs,
                     const int32_t *d_jobs, double *d_P, double *d_out, void *stream) {
  if (rows < 0 || N < 0 || T < 0 || n_jobs < 0)
    return fail(FR_E_ARG, "fr_arctic_argmax: bad shape");
  if (rows == 0 || N == 0 || T == 0 || n_jobs == 0) return FR_OK;
  if (!d_V || !d_jobs || !d_P || !d_out)
    return fail(FR_E_ARG, "fr_arctic_argmax: null device pointer");
  hipError_t e = fr::launch_arctic_argmax(d_V, rows, N, T, n_jobs, d_jobs, d_P, d_out,
                                          (hipStream_t)stream);
  return launched(e, "arctic argmax launch", "fr_arctic_argmax: grid too large (rows * N, N or jobs)");
}

int fr_nan_to_num(double *d_x, int64_t count, void *stream) {
  if (count < 0) return fail(FR_E_ARG, "fr_nan_to_num: bad count");
  if (count == 0) return FR_OK;
  if (!d_x) return fail(FR_E_ARG, "fr_nan_to_num: null device pointer");
  hipError_t e = fr::launch_nan_to_num(d_x, count, (hipStream_t)stream);
  return launched(e, "nan_to_num launch");
}

int fr_coswiss_combine(const double *d_terms, int64_t n_terms, int64_t N, int64_t T,
                       int32_t n_out, const int32_t *d_begin, const double *d_coeff,
                       const int32_t *d_desc, const double *d_trig, double *d_out,
                       int64_t out_row_stride, void *stream) {
  if (n_terms < 0 || N < 0 || T < 0 || n_out < 0)
    return fail(FR_E_ARG, "fr_coswiss_combine: bad shape");
  if (N == 0 || T == 0 || n_out == 0) return FR_OK;
  if (N * (int64_t)n_out > 0x7fffffffLL) return fail(FR_E_LIMIT, "fr_coswiss_combine: grid too large");
  if (out_row_stride < N * T) return fail(FR_E_ARG, "fr_coswiss_combine: rows of d_out overlap");
  if (!d_terms || !d_begin || !d_coeff || !d_desc || !d_trig || !d_out)
    return fail(FR_E_ARG, "fr_coswiss_combine: null device pointer");
  hipError_t e = fr::launch_coswiss_combine(d_terms, N, T, n_out, d_begin, d_coeff, d_desc, d_trig,
                                            d_out, out_row_stride, (hipStream_t)stream);
  return launched(e, "coswiss combine launch");
}

// ---------------------------------------------------------------- preparateurs (kernels_prep.hip)
int fr_prep_fir(const double *d_X, int64_t N, int64_t D, int64_t T, const double *d_kernel,
                int32_t J, int32_t w, const int32_t *d_ndim, int32_t O, const int32_t *d_dims,
                const int32_t *h_ndim, const int32_t *h_dims, int32_t mode, int32_t adaptive,
                double *d_out, void *stream) {
  if (N < 0 || D < 1 || T < 1 || w < 0 || (mode != 0 && mode != 1))
    return fail(FR_E_ARG, "fr_prep_fir: bad shape");
  if (mode == 1) {
    if (w < 1 || w > T) return fail(FR_E_ARG, "fr_prep_fir: a moving average wider than the series");
    O = (int32_t)D;
    if (D > 0x7fffffffLL) return fail(FR_E_LIMIT, "fr_prep_fir: too many dimensions");
  } else {
    if (J < 1 || O < 1 || J > D)
      return fail(FR_E_ARG, "fr_prep_fir: 1 <= slots <= D (slot j adds dimension j itself)");
    if (!adaptive && w >= T) return fail(FR_E_ARG, "fr_prep_fir: the kernel must be shorter than the series");
    const int rc = check_groups("fr_prep_fir", h_ndim, O, h_dims, J, D);
    if (rc != FR_OK) return rc;
    if ((w > 0 && !d_kernel) || !d_ndim || !d_dims)
      return fail(FR_E_ARG, "fr_prep_fir: null device pointer");
  }
  if (N == 0) return FR_OK;
  if (!d_X || !d_out || d_X == d_out) return fail(FR_E_ARG, "fr_prep_fir: null or aliased device pointer");
  hipError_t e = fr::launch_prep_fir(d_X, N, D, T, d_kernel, w, d_ndim, O, d_dims, mode,
                                     adaptive ? 1 : 0, d_out, (hipStream_t)stream);
  return launched(e, "prep fir launch", "fr_prep_fir: grid too large");
}

int fr_prep_project(const double *d_X, int64_t N, int64_t D, int64_t T, const double *d_kernel,
                    const double *d_bias, const int32_t *d_ndim, int32_t O, const int32_t *d_dims,
                    int32_t J, const int32_t *h_ndim, const int32_t *h_dims, const double *d_W1,
                    const double *d_b1, const double *d_W2, int32_t hidden, int32_t flags,
                    double *d_out, void *stream) {
  if (N < 0 || D < 1 || T < 1 || O < 1 || hidden < 0 || D > 0x7fffffffLL)
    return fail(FR_E_ARG, "fr_prep_project: bad shape");
  if (hidden == 0) {
    if (J < 0) return fail(FR_E_ARG, "fr_prep_project: bad shape");
    const int rc = check_groups("fr_prep_project", h_ndim, O, h_dims, J, D);
    if (rc != FR_OK) return rc;
    if (!d_kernel || !d_bias || !d_ndim || !d_dims)
      return fail(FR_E_ARG, "fr_prep_project: null device pointer");
  } else {
    if (D > 16 || O > 16)
      return fail(FR_E_LIMIT, "fr_prep_project: a hidden layer between at most 16 input and 16 output dimensions");
    if (!d_W1 || !d_b1 || !d_W2) return fail(FR_E_ARG, "fr_prep_project: null device pointer");
  }
  if (N == 0) return FR_OK;
  if (!d_X || !d_out || d_X == d_out) return fail(FR_E_ARG, "fr_prep_project: null or aliased device pointer");
  hipError_t e = fr::launch_prep_project(d_X, N, D, T, d_kernel, d_bias, d_ndim, O, d_dims, d_W1, d_b1,
                                         d_W2, hidden, flags, d_out, (hipStream_t)stream);
  return launched(e, "prep project launch", "fr_prep_project: grid too large");
}

int fr_prep_normalize(const double *d_X, int64_t N, int64_t D, int64_t T, int32_t scale_dim,
                      double *d_out, void *stream) {
  if (N < 0 || D < 1 || T < 1) return fail(FR_E_ARG, "fr_prep_normalize: bad shape");
  if (N == 0) return FR_OK;
  if (!d_X || !d_out || d_X == d_out) return fail(FR_E_ARG, "fr_prep_normalize: null or aliased device pointer");
  hipError_t e = scale_dim ? fr::launch_prep_normalize(d_X, N, D * T, d_out, (hipStream_t)stream)
                           : fr::launch_prep_normalize(d_X, N * D, T, d_out, (hipStream_t)stream);
  return launched(e, "prep normalize launch", "fr_prep_normalize: grid too large");
}

int fr_prep_leadlag(const double *d_X, int64_t N, int64_t D, int64_t T, double *d_out,
                    void *stream) {
  if (N < 0 || D < 1 || T < 1) return fail(FR_E_ARG, "fr_prep_leadlag: bad shape");
  if (N == 0) return FR_OK;
  if (!d_X || !d_out || d_X == d_out) return fail(FR_E_ARG, "fr_prep_leadlag: null or aliased device pointer");
  hipError_t e = fr::launch_prep_leadlag(d_X, N * D, T, d_out, (hipStream_t)stream);
  return launched(e, "prep leadlag launch", "fr_prep_leadlag: grid too large");
}

// ---------------------------------------------------------------- streaming preparateurs (kernels_filter.hip)
int fr_prep_mask(const double *d_X, int64_t N, int64_t D, int64_t T, const uint32_t *d_mask,
                 int64_t mask_words, const int64_t *d_cs, const int64_t *d_ce, int64_t n_windows,
                 double *d_out, void *stream) {
  if (N < 0 || D < 1 || T < 1) return fail(FR_E_ARG, "fr_prep_mask: bad shape");
  if (d_mask && mask_words != (T + 31) / 32)
    return fail(FR_E_ARG, "fr_prep_mask: the time mask has to hold ceil(T / 32) words");
  if ((d_cs == nullptr) != (d_ce == nullptr))
    return fail(FR_E_ARG, "fr_prep_mask: a window needs both its start and its end counts");
  if (d_cs && n_windows < N)
    return fail(FR_E_ARG, "fr_prep_mask: fewer windows than series");
  if (N == 0) return FR_OK;
  if (!d_X || !d_out || d_X == d_out) return fail(FR_E_ARG, "fr_prep_mask: null or aliased device pointer");
  hipError_t e = fr::launch_prep_mask(d_X, N, D, T, d_mask, d_cs, d_ce, d_out, (hipStream_t)stream);
  return launched(e, "prep mask launch", "fr_prep_mask: grid too large");
}

int fr_prep_pointwise(int32_t mode, const double *d_X, int64_t Nx, int64_t D, int64_t T,
                      const double *d_w, int64_t Nw, const double *d_w2, int64_t shift, double q,
                      double v, int32_t flags, double *d_out, void *stream) {
  if (mode < FR_PW_MUL || mode > FR_PW_CLIP) return fail(FR_E_ARG, "fr_prep_pointwise: unknown mode");
  if (Nx < 0 || D < 1 || T < 1) return fail(FR_E_ARG, "fr_prep_pointwise: bad shape");
  int64_t N = Nx;
  fr::PointwiseArgs a{};
  a.X = d_X;
  a.out = d_out;
  a.D = D;
  a.T = T;
  a.x_stride = D * T;
  a.flags = flags;
  if (mode == FR_PW_MUL || mode == FR_PW_ADD) {
    if (Nw < 0) return fail(FR_E_ARG, "fr_prep_pointwise: bad shape");
    if (Nx != Nw && Nx != 1 && Nw != 1)
      return fail(FR_E_ARG, "fr_prep_pointwise: " + std::to_string(Nx) + " series do not broadcast against " +
                                std::to_string(Nw) + " table rows");
    N = (Nx == 0 || Nw == 0) ? 0 : (Nx > Nw ? Nx : Nw);
    if (N > 0 && !d_w) return fail(FR_E_ARG, "fr_prep_pointwise: null device pointer");
    a.w = d_w;
    a.x_stride = Nx == 1 ? 0 : D * T;
    a.w_stride = Nw == 1 ? 0 : T;
  } else if (mode == FR_PW_ROTATE) {
    if (D != 2) return fail(FR_E_ARG, "fr_prep_pointwise: a rotation needs exactly 2 dimensions");
    if (N > 0 && (!d_w || !d_w2)) return fail(FR_E_ARG, "fr_prep_pointwise: null device pointer");
    a.w = d_w;
    a.w2 = d_w2;
  } else if (mode == FR_PW_POW) {
    if (N > 0 && !d_w) return fail(FR_E_ARG, "fr_prep_pointwise: null device pointer");
    a.w = d_w;
  } else if (mode == FR_PW_SHIFT) {
    if (shift < 0) return fail(FR_E_ARG, "fr_prep_pointwise: negative shift");
    a.shift = shift < T ? shift : T;
  } else {
    a.q = q;
    a.v = v;
  }
  if (N == 0) return FR_OK;
  if (!d_X || !d_out || d_X == d_out)
    return fail(FR_E_ARG, "fr_prep_pointwise: null or aliased device pointer");
  hipError_t e = fr::launch_prep_pointwise(mode, a, N, (hipStream_t)stream);
  return launched(e, "prep pointwise launch", "fr_prep_pointwise: grid too large");
}

// ---------------------------------------------------------------- generic words (kernels_letters.hip)
namespace {
// whether the doubles [a, a + na) and [b, b + nb) share an address
bool overlap(const double *a, int64_t na, const double *b, int64_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + (uintptr_t)nb * sizeof(double) && pb < pa + (uintptr_t)na * sizeof(double);
}
}  // namespace

int fr_letter_rows(const double *d_X, int64_t N, int64_t D, int64_t T, const double *d_ext,
                   int64_t H, const int32_t *d_spec, const int32_t *h_spec, int32_t Dv,
                   int32_t one_is_zero, double *d_out, void *stream) {
  if (N < 0 || D < 1 || T < 1 || H < 0 || Dv < 1) return fail(FR_E_ARG, "fr_letter_rows: bad shape");
  if (!h_spec) return fail(FR_E_ARG, "fr_letter_rows: null host table");
  for (int32_t r = 0; r < Dv; ++r) {
    const int32_t kind = h_spec[3 * r], source = h_spec[3 * r + 1], shift = h_spec[3 * r + 2];
    const std::string row = "fr_letter_rows: row " + std::to_string(r);
    if (kind < FR_ROW_DIM || kind > FR_ROW_ONE) return fail(FR_E_ARG, row + " has an unknown kind");
    if (shift < 0) return fail(FR_E_ARG, row + " has a negative shift");
    if (kind == FR_ROW_ONE) continue;
    if (kind == FR_ROW_EXT && (!d_ext || H == 0))
      return fail(FR_E_ARG, row + " reads letter values but there are none");
    const int64_t limit = kind == FR_ROW_EXT ? H : D;
    if (source < 0 || source >= limit)
      return fail(FR_E_DIM, row + " names source " + std::to_string(source) + " of " +
                                std::to_string(limit));
  }
  if (N == 0) return FR_OK;
  if (!d_X || !d_out || !d_spec) return fail(FR_E_ARG, "fr_letter_rows: null or aliased device pointer");
  if (overlap(d_X, N * D * T, d_out, N * Dv * T) ||
      (d_ext && H > 0 && overlap(d_ext, N * H * T, d_out, N * Dv * T)))
    return fail(FR_E_ARG, "fr_letter_rows: null or aliased device pointer");
  hipError_t e = fr::launch_letter_rows(d_X, N, D, T, d_ext, H, d_spec, Dv, one_is_zero ? 0.0 : 1.0,
                                        d_out, (hipStream_t)stream);
  return launched(e, "letter rows launch", "fr_letter_rows: grid too large");
}

int fr_rows_unshift(const double *d_A, int64_t K, int64_t N, int64_t T, const int32_t *d_shift,
                    const int32_t *h_shift, double *d_out, void *stream) {
  if (K < 0 || N < 0 || T < 1) return fail(FR_E_ARG, "fr_rows_unshift: bad shape");
  if (K > 0 && !h_shift) return fail(FR_E_ARG, "fr_rows_unshift: null host table");
  for (int64_t k = 0; k < K; ++k)
    if (h_shift[k] < 0)
      return fail(FR_E_ARG, "fr_rows_unshift: row " + std::to_string(k) + " has a negative shift");
  if (K == 0 || N == 0) return FR_OK;
  if (!d_A || !d_out || !d_shift || overlap(d_A, K * N * T, d_out, K * N * T))
    return fail(FR_E_ARG, "fr_rows_unshift: null or aliased device pointer");
  hipError_t e = fr::launch_rows_unshift(d_A, K, N, T, d_shift, d_out, (hipStream_t)stream);
  return launched(e, "rows unshift launch", "fr_rows_unshift: grid too large");
}

int fr_sieve_pick(const double *d_A, int64_t K, int64_t N, int64_t T, const int32_t *d_spec,
                  const int32_t *h_spec, int32_t n_sieves, const int64_t *d_cuts, int64_t n_cuts,
                  const double *d_q, int64_t n_q, int32_t F, double *d_feat, int32_t *d_pos,
                  void *stream) {
  const std::string who = "fr_sieve_pick";
  if (K < 0 || N < 0 || T < 1 || n_sieves < 1 || n_cuts < 0 || n_q < 0 || F < 1)
    return fail(FR_E_ARG, who + ": bad shape");
  if (F > fr::kPickMaxFeatures)
    return fail(FR_E_LIMIT, who + ": at most 256 features per row, not " + std::to_string(F));
  if (T > 0x7fffffffLL) return fail(FR_E_LIMIT, who + ": positions are 32-bit, T is not");
  if (!h_spec) return fail(FR_E_ARG, who + ": null host table");
  // per-series cuts: every sieve or none; d_cuts is then (N, n_cuts / N) and a sieve's cut row
  // lies within a series' row
  const bool series_cuts = (h_spec[0] & FR_SIEVE_SERIES_CUTS) != 0;
  for (int32_t s = 1; s < n_sieves; ++s)
    if (((h_spec[6 * (int64_t)s] & FR_SIEVE_SERIES_CUTS) != 0) != series_cuts)
      return fail(FR_E_ARG, who + ": sieve " + std::to_string(s) + " and sieve 0 differ in FR_SIEVE_SERIES_CUTS: "
                                  "either every sieve reads per-series cuts or none does");
  if (series_cuts && N > 0 && n_cuts % N != 0)
    return fail(FR_E_ARG, who + ": per-series cuts are an (N, row) table, but n_cuts = " +
                              std::to_string(n_cuts) + " is no multiple of N = " + std::to_string(N));
  const int64_t cut_row = series_cuts && N > 0 ? n_cuts / N : n_cuts;
  // every entry of the table, before a kernel reads the device copy
  int64_t features = 0;
  for (int32_t s = 0; s < n_sieves; ++s) {
    const int32_t *sp = h_spec + 6 * (int64_t)s;
    const std::string sieve = who + ": sieve " + std::to_string(s);
    const int32_t kind = sp[0] & ~FR_SIEVE_SERIES_CUTS, cut_begin = sp[1], C1 = sp[2], q_begin = sp[3], Q1 = sp[4];
    if (kind != FR_SIEVE_END && kind != FR_SIEVE_MAX && kind != FR_SIEVE_MIN)
      return fail(FR_E_ARG, sieve + " is no selecting sieve (END, MAX, MIN): kind " + std::to_string(kind));
    if (C1 < 2 || cut_begin < 0 || (int64_t)cut_begin + C1 > cut_row)
      return fail(FR_E_ARG, sieve + (series_cuts ? " has a cut row outside a series' row of the cut table"
                                                 : " has a cut row outside the cut table"));
    if (kind != FR_SIEVE_END && (Q1 < 2 || q_begin < 0 || (int64_t)q_begin + Q1 > n_q))
      return fail(FR_E_ARG, sieve + " has thresholds outside the threshold table");
    if (sp[5] != features)
      return fail(FR_E_ARG, sieve + " begins at feature " + std::to_string(sp[5]) + ", not at " +
                                std::to_string(features));
    features += (int64_t)(C1 - 1) * (kind == FR_SIEVE_END ? 1 : Q1 - 1);
    if (features > F) break;
  }
  if (features != F)
    return fail(FR_E_ARG, who + ": the sieves have " + std::string(features > F ? "more than " : "") +
                              std::to_string(features > F ? F : features) + " features, not F = " + std::to_string(F));
  if (K == 0 || N == 0) return FR_OK;
  if (!d_A || !d_spec || !d_cuts || !d_feat || !d_pos || (n_q > 0 && !d_q))
    return fail(FR_E_ARG, who + ": null device pointer");
  hipError_t e = fr::launch_sieve_pick(d_A, K, N, T, reinterpret_cast<const fr::PickSieve *>(d_spec), n_sieves,
                                       d_cuts, series_cuts ? cut_row : 0, d_q, F, d_feat, d_pos,
                                       (hipStream_t)stream);
  return launched(e, "sieve pick launch", "fr_sieve_pick: grid too large (K * N)");
}

// ---------------------------------------------------------------- band heads (kernels_heads.hip)
namespace {
// The shapes and every entry of the (n_sieves, 7) spec table of fr_sieve_heads[_adjoint], before
// a kernel reads the device copy: FR_OK, or the failure.  *cut_stride: the cut table's row per
// series with per-series cuts, else 0.
int check_heads(const std::string &who, int64_t K, int64_t N, int64_t T, const int32_t *h_spec,
                int32_t n_sieves, int64_t n_cuts, int64_t n_q, int32_t F, int64_t *cut_stride) {
  if (K < 0 || N < 0 || T < 1 || n_sieves < 1 || n_cuts < 0 || n_q < 0 || F < 1)
    return fail(FR_E_ARG, who + ": bad shape");
  if (F > fr::kPickMaxFeatures)
    return fail(FR_E_LIMIT, who + ": at most 256 features per row, not " + std::to_string(F));
  if (T > 0x7fffffffLL) return fail(FR_E_LIMIT, who + ": positions and counts are 32-bit, T is not");
  if (!h_spec) return fail(FR_E_ARG, who + ": null host table");
  const bool series_cuts = (h_spec[0] & FR_SIEVE_SERIES_CUTS) != 0;
  for (int32_t s = 1; s < n_sieves; ++s)
    if (((h_spec[7 * (int64_t)s] & FR_SIEVE_SERIES_CUTS) != 0) != series_cuts)
      return fail(FR_E_ARG, who + ": sieve " + std::to_string(s) + " and sieve 0 differ in FR_SIEVE_SERIES_CUTS: "
                                  "either every sieve reads per-series cuts or none does");
  if (series_cuts && N > 0 && n_cuts % N != 0)
    return fail(FR_E_ARG, who + ": per-series cuts are an (N, row) table, but n_cuts = " +
                              std::to_string(n_cuts) + " is no multiple of N = " + std::to_string(N));
  const int64_t cut_row = series_cuts && N > 0 ? n_cuts / N : n_cuts;
  int64_t features = 0;
  for (int32_t s = 0; s < n_sieves; ++s) {
    const int32_t *sp = h_spec + 7 * (int64_t)s;
    const std::string sieve = who + ": sieve " + std::to_string(s);
    const int32_t kind = sp[0] & ~FR_SIEVE_SERIES_CUTS, cut_begin = sp[1], C1 = sp[2], q_begin = sp[3], Q1 = sp[4];
    const bool selects = kind == FR_SIEVE_END || kind == FR_SIEVE_MAX || kind == FR_SIEVE_MIN;
    if (!selects && kind != FR_SIEVE_MPI && kind != FR_SIEVE_CUR)
      return fail(FR_E_ARG, sieve + " is no head (END, MAX, MIN, MPI, CUR): kind " + std::to_string(kind));
    const int32_t lo = kind == FR_SIEVE_CUR ? 2 : 0,
                  hi = kind == FR_SIEVE_CUR ? 2 : (kind == FR_SIEVE_MPI ? fr::kMaxInc : 0);
    if (sp[6] < lo || sp[6] > hi)
      return fail(FR_E_ARG, sieve + " has the differencing order " + std::to_string(sp[6]) + ", not " +
                                (lo == hi ? std::to_string(lo) : "0 ... 8"));
    if (C1 < 2 || cut_begin < 0 || (int64_t)cut_begin + C1 > cut_row)
      return fail(FR_E_ARG, sieve + (series_cuts ? " has a cut row outside a series' row of the cut table"
                                                 : " has a cut row outside the cut table"));
    if (kind != FR_SIEVE_END && (Q1 < 2 || q_begin < 0 || (int64_t)q_begin + Q1 > n_q))
      return fail(FR_E_ARG, sieve + " has thresholds outside the threshold table");
    if (sp[5] != features)
      return fail(FR_E_ARG, sieve + " begins at feature " + std::to_string(sp[5]) + ", not at " +
                                std::to_string(features));
    features += (int64_t)(C1 - 1) * (kind == FR_SIEVE_END ? 1 : Q1 - 1);
    if (features > F) break;
  }
  if (features != F)
    return fail(FR_E_ARG, who + ": the sieves have " + std::string(features > F ? "more than " : "") +
                              std::to_string(features > F ? F : features) + " features, not F = " + std::to_string(F));
  *cut_stride = series_cuts ? cut_row : 0;
  return FR_OK;
}
}  // namespace

int fr_sieve_heads(const double *d_A, int64_t K, int64_t N, int64_t T, const int32_t *d_spec,
                   const int32_t *h_spec, int32_t n_sieves, const int64_t *d_cuts, int64_t n_cuts,
                   const double *d_q, int64_t n_q, int32_t F, double *d_feat, int32_t *d_comp,
                   void *hip_stream) {
  const std::string who = "fr_sieve_heads";
  int64_t cut_stride = 0;
  if (int rc = check_heads(who, K, N, T, h_spec, n_sieves, n_cuts, n_q, F, &cut_stride)) return rc;
  if (K == 0 || N == 0) return FR_OK;
  if (!d_A || !d_spec || !d_cuts || !d_feat || !d_comp || (n_q > 0 && !d_q))
    return fail(FR_E_ARG, who + ": null device pointer");
  hipError_t e = fr::launch_sieve_heads(d_A, K, N, T, reinterpret_cast<const fr::HeadSieve *>(d_spec), n_sieves,
                                        d_cuts, cut_stride, d_q, F, d_feat, d_comp, (hipStream_t)hip_stream);
  return launched(e, "sieve heads launch", "fr_sieve_heads: grid too large (K * N)");
}

int fr_sieve_heads_adjoint(const double *d_rows, int64_t V, const int32_t *d_row_map,
                           const int32_t *h_row_map, int64_t K, int64_t N, int64_t T,
                           const int32_t *d_spec, const int32_t *h_spec, int32_t n_sieves,
                           const int64_t *d_cuts, int64_t n_cuts, const double *d_q, int64_t n_q, int32_t F,
                           const int32_t *d_comp, const double *d_g, const int32_t *d_lengths, double *d_G,
                           void *hip_stream) {
  const std::string who = "fr_sieve_heads_adjoint";
  int64_t cut_stride = 0;
  if (V < 0) return fail(FR_E_ARG, who + ": bad shape");
  if (int rc = check_heads(who, K, N, T, h_spec, n_sieves, n_cuts, n_q, F, &cut_stride)) return rc;
  // the row map: both copies or neither; without one the buffer holds the K rows themselves
  if ((d_row_map != nullptr) != (h_row_map != nullptr))
    return fail(FR_E_ARG, who + ": the row map needs its host and its device copy");
  if (!h_row_map && V != K)
    return fail(FR_E_ARG, who + ": without a row map the buffer holds the K = " + std::to_string(K) +
                              " rows, not V = " + std::to_string(V));
  for (int64_t k = 0; h_row_map && k < K; ++k)
    if (h_row_map[k] < 0 || h_row_map[k] >= V)
      return fail(FR_E_ARG, who + ": row " + std::to_string(k) + " names row " + std::to_string(h_row_map[k]) +
                                " of " + std::to_string(V));
  if (K == 0 || N == 0) return FR_OK;
  if (!d_rows || !d_spec || !d_cuts || !d_comp || !d_g || !d_G || (n_q > 0 && !d_q))
    return fail(FR_E_ARG, who + ": null device pointer");
  if (overlap(d_rows, V * N * T, d_G, K * N * T) || overlap(d_g, K * N * F, d_G, K * N * T))
    return fail(FR_E_ARG, who + ": d_G must not alias the rows or the feature gradients");
  hipError_t e = fr::launch_sieve_heads_adjoint(d_rows, d_row_map, K, N, T,
                                                reinterpret_cast<const fr::HeadSieve *>(d_spec), n_sieves, d_cuts,
                                                cut_stride, d_q, F, d_comp, d_g, d_lengths, d_G,
                                                (hipStream_t)hip_stream);
  return launched(e, "sieve heads adjoint launch", "fr_sieve_heads_adjoint: grid too large (K * N)");
}

}  // extern "C"

// Micro-benchmark: the practical ceiling of the walk kernel's TRAFFIC MIX on MI355X - a kernel
// that moves exactly the headline's bytes in the walk's shape and does nothing else: per unit
// (series n, group g of G) read the series' 3 rows (24 KB) and write K / G output rows of 8 KB to
// out[k][n][:], one workgroup per unit or a persistent grid.
//
// Axes: read mode (none, plain, non-temporal loads) x groups per series x cache policy of the
// 16-byte output stores (a plain global store, or a buffer store with the policy bits plain, sc1,
// sc0 sc1, nt, nt sc1).  Every cell is timed back to back (10 launches between one event pair)
// and isolated (each launch between its own event pair, the device drained in front of it).
//   hipcc --offload-arch=gfx950 -O3 tools/stream_mix.hip -o /tmp/sm && /tmp/sm [--persistent | --tail]
// --tail: the headline batch with its last series moved in third-units (the walk's mixed launch)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include <algorithm>

typedef double vd2 __attribute__((ext_vector_type(2)));
typedef unsigned int vu4 __attribute__((ext_vector_type(4)));
constexpr int T = 1024, D = 3, K = 18;

// store policies: -1 = plain global store; otherwise the aux (cache policy) operand of a buffer
// store on gfx950: 0 plain, 1 sc0, 2 nt, 16 sc1, 17 sc0 sc1, 18 nt sc1
constexpr int kPolicies[] = {-1, 0, 16, 17, 2, 18};
static const char *policy_name(int p) {
  switch (p) {
    case -1: return "global plain";
    case 0: return "buf plain";
    case 16: return "buf sc1";
    case 17: return "buf sc0 sc1";
    case 2: return "buf nt";
    case 18: return "buf nt sc1";
  }
  return "?";
}

template <int G, int READ, int POL>   // READ 0: no input, 1: plain loads, 2: non-temporal loads
__global__ __launch_bounds__(256) void mix_kernel(const double *X, double *out, int N) {
  const int tid = threadIdx.x;
  const int units = N * G;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int q = u >> 3, r = u & 7;
    const int n = (q / G) * 8 + r, g = q % G;
    vd2 v[D][2];
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
      for (int k = 0; k < 2; ++k)
      {
        const vd2 *src = reinterpret_cast<const vd2 *>(X + ((size_t)n * D + d) * T + 2 * (k * 256 + tid));
        if constexpr (READ == 0) v[d][k] = vd2{(double)n, (double)tid};
        else if constexpr (READ == 1) v[d][k] = *src;
        else v[d][k] = __builtin_nontemporal_load(src);
      }
#pragma unroll
    for (int j = 0; j < K / G; ++j) {
      const int k = g * (K / G) + j;
      double *dst = out + ((size_t)k * N + n) * T;
      if constexpr (POL < 0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          vd2 w = v[j % D][h];
          w.x += (double)j;
          *reinterpret_cast<vd2 *>(dst + 2 * (h * 256 + tid)) = w;
        }
      } else {
        // one descriptor per row (the row pointer is uniform); num_records = the row's bytes
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(dst, 0, T * 8, 0x00020000);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          vd2 w = v[j % D][h];
          w.x += (double)j;
          vu4 bits;
          __builtin_memcpy(&bits, &w, 16);
          __builtin_amdgcn_raw_buffer_store_b128(bits, rs, 16 * (h * 256 + tid), 0, POL);
        }
      }
    }
  }
}

// The same bytes with the last N - n_whole series in finer units: workgroup b < n_whole moves
// series b whole (non-temporal loads, K planes); the workgroups behind are three movers per
// series of K / 3 planes each, which all read the 3 rows again with plain loads (the XCD-aware
// numbering of the walk: the movers of one series meet in one L2).  sc1 stores throughout.
// n_whole = N is the unsplit mover (G = 1, nt reads, sc1).
__global__ __launch_bounds__(256) void mix_tail_kernel(const double *X, double *out, int N, int n_whole) {
  const int tid = threadIdx.x, b = blockIdx.x;
  int n = b, k0 = 0, k1 = K;
  const bool whole = b < n_whole;
  if (!whole) {
    const int j = b - n_whole, q = j >> 3, r = j & 7;   // (N - n_whole is a multiple of 8 here)
    n = n_whole + (q / 3) * 8 + r;
    k0 = (q % 3) * (K / 3);
    k1 = k0 + K / 3;
  }
  vd2 v[D][2];
#pragma unroll
  for (int d = 0; d < D; ++d)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const vd2 *src = reinterpret_cast<const vd2 *>(X + ((size_t)n * D + d) * T + 2 * (k * 256 + tid));
      v[d][k] = whole ? __builtin_nontemporal_load(src) : *src;
    }
  for (int k = k0; k < k1; ++k) {
    double *dst = out + ((size_t)k * N + n) * T;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(dst, 0, T * 8, 0x00020000);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      vd2 w = v[0][h] + v[1][h] + v[2][h];
      w.x += (double)k;
      vu4 bits;
      __builtin_memcpy(&bits, &w, 16);
      __builtin_amdgcn_raw_buffer_store_b128(bits, rs, 16 * (h * 256 + tid), 0, 16);
    }
  }
}

// median back-to-back time (us) of the split mover, 7 batches of 10 launches
static float run_tail(const double *X, double *out, int N, int n_whole) {
  hipEvent_t a, b;
  hipEventCreate(&a); hipEventCreate(&b);
  const int g = n_whole + 3 * (N - n_whole);
  auto launch = [&] { hipLaunchKernelGGL(mix_tail_kernel, dim3(g), dim3(256), 0, 0, X, out, N, n_whole); };
  for (int w = 0; w < 5; ++w) launch();
  std::vector<float> ts;
  for (int r = 0; r < 7; ++r) {
    hipEventRecord(a);
    for (int rep = 0; rep < 10; ++rep) launch();
    hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b); ts.push_back(ms / 10);
  }
  std::sort(ts.begin(), ts.end());
  hipEventDestroy(a); hipEventDestroy(b);
  return ts[3] * 1e3f;
}

struct Cell { float b2b, iso; };

template <int G, int READ, int POL>
static Cell run(const double *X, double *out, int N, int grid) {
  hipEvent_t a, b;
  hipEventCreate(&a); hipEventCreate(&b);
  const int g = grid ? grid : N * G;
  auto launch = [&] { hipLaunchKernelGGL((mix_kernel<G, READ, POL>), dim3(g), dim3(256), 0, 0, X, out, N); };
  for (int w = 0; w < 5; ++w) launch();
  std::vector<float> ts, iso;
  for (int r = 0; r < 7; ++r) {
    hipEventRecord(a);
    for (int rep = 0; rep < 10; ++rep) launch();
    hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b); ts.push_back(ms / 10);
  }
  for (int r = 0; r < 21; ++r) {
    hipDeviceSynchronize();
    hipEventRecord(a);
    launch();
    hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b); iso.push_back(ms);
  }
  std::sort(ts.begin(), ts.end());
  std::sort(iso.begin(), iso.end());
  hipEventDestroy(a); hipEventDestroy(b);
  return {ts[3] * 1e3f, iso[10] * 1e3f};
}

template <int G, int READ>
static void row(const double *X, double *out, int N, int grid) {
  static const char *rn[] = {"writes only", "reads + writes", "nt reads + writes"};
  constexpr int NP = sizeof(kPolicies) / sizeof(int);
  // three interleaved passes over the policies; the median pass per cell
  std::vector<Cell> c[NP];
  for (int pass = 0; pass < 3; ++pass) {
    c[0].push_back(run<G, READ, -1>(X, out, N, grid));
    c[1].push_back(run<G, READ, 0>(X, out, N, grid));
    c[2].push_back(run<G, READ, 16>(X, out, N, grid));
    c[3].push_back(run<G, READ, 17>(X, out, N, grid));
    c[4].push_back(run<G, READ, 2>(X, out, N, grid));
    c[5].push_back(run<G, READ, 18>(X, out, N, grid));
  }
  const double bytes = 8.0 * N * T * ((READ ? D : 0) + K);
  for (int p = 0; p < NP; ++p) {
    std::vector<float> b2b, iso;
    for (auto &x : c[p]) { b2b.push_back(x.b2b); iso.push_back(x.iso); }
    std::sort(b2b.begin(), b2b.end()); std::sort(iso.begin(), iso.end());
    printf("N %5d  G %d  %-18s %-13s %s: b2b %7.1f us (%.2f TB/s)  isolated %7.1f us   [%4.0f MB]\n",
           N, G, rn[READ], policy_name(kPolicies[p]), grid ? "persistent" : "per unit  ",
           b2b[1], bytes / (b2b[1] * 1e-6) / 1e12, iso[1], bytes / 1e6);
  }
  fflush(stdout);
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "--tail")) {
    // the headline batch, unsplit against the last N - n_whole series in third-units: three
    // interleaved passes, every time printed
    const int N = 2048;
    double *X, *out;
    hipMalloc(&X, (size_t)N * D * T * 8);
    hipMalloc(&out, (size_t)K * N * T * 8);
    hipMemset(X, 0, (size_t)N * D * T * 8);
    for (int pass = 0; pass < 3; ++pass)
      for (int n_whole : {2048, 1792, 1536, 1280, 0})
        printf("pass %d  N %d  n_whole %4d  grid %4d: b2b %6.1f us\n", pass, N, n_whole,
               n_whole + 3 * (N - n_whole), run_tail(X, out, N, n_whole));
    hipFree(X); hipFree(out);
    return 0;
  }
  const int grid = (argc > 1 && !strcmp(argv[1], "--persistent")) ? 1536 : 0;
  for (int N : {2048, 1536, 3072, 8192}) {
    double *X, *out;
    hipMalloc(&X, (size_t)N * D * T * 8);
    hipMalloc(&out, (size_t)K * N * T * 8);
    hipMemset(X, 0, (size_t)N * D * T * 8);
    row<1, 0>(X, out, N, grid);
    row<1, 1>(X, out, N, grid);
    row<1, 2>(X, out, N, grid);
    row<3, 0>(X, out, N, grid);
    row<3, 1>(X, out, N, grid);
    row<3, 2>(X, out, N, grid);
    hipFree(X); hipFree(out);
  }
  return 0;
}

// Micro-benchmark of tools/kernarg_floor.py: what does a serial scalar round trip to the cold
// kernel-argument segment cost at kernel start?  One captured graph of N dependent launches of
// a row gather (R rows of F floats through a permutation, reading the previous launch's
// output), in four forms that differ only in how the wave gets its arguments:
//   0 lazy     a 408-byte struct by value, read at three dependent points (flag -> count ->
//              pointers), each field in another 64-byte line -- what k_hop did
//   1 pinned   the same struct, every field named at kernel entry: one round trip
//   2 preload  the entry fields as leading scalar parameters (built with
//              -mllvm -amdgpu-kernarg-preload-count=16: they arrive in SGPRs), the rest a struct
//   3 pointer  one pointer argument, everything else compile-time: the floor
// kf_run(variant, n, reps, &us_per_launch) returns a hipError_t.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
constexpr int R = 10369, F = 32, kThreads = 256;
constexpr int kGrid = (R * (F / 4) + kThreads - 1) / kThreads;

// 408 bytes like HopArgs; the entry fields sit where k_hop's do (xcd 0x3c, recs 0x58, ntiles
// 0x60, in / out 0x68..0x88)
struct Args {
  int pad0[15];
  int xcd;  // 0x3c
  int pad1[6];
  const int* perm;  // 0x58
  int rows;         // 0x60
  int pad2;
  const float* in;  // 0x68
  int pad3[6];
  float* out;       // 0x88
  int tail[66];
};
static_assert(sizeof(Args) == 408, "the middle hop's argument bytes");
struct Rest {
  int tail[90];
};

__device__ __forceinline__ void gather(const int* perm, const float* in, float* out, int rows) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int r = i / (F / 4), q = i % (F / 4);
  if (r >= rows) return;
  const float4 v = reinterpret_cast<const float4*>(in + (size_t)perm[r] * F)[q];
  reinterpret_cast<float4*>(out + (size_t)r * F)[q] = v;
}
// a zero the compiler cannot see through, available only once v has arrived: an argument read
// at an offset that includes it stays behind v's round trip, as the reads behind k_hop's
// branches do
__device__ __forceinline__ int zero_after(int v) {
  int z = 0;
  asm volatile("" : "+s"(z) : "s"(v));
  return z;
}
__global__ __launch_bounds__(kThreads) void k_lazy(Args a) {
  const char* base = reinterpret_cast<const char*>(&a);
  const int x = a.xcd;  // trip 1
  if (x > 0 && (int)(blockIdx.x % 8) >= x) return;
  const int rows = *reinterpret_cast<const int*>(base + 0x60 + zero_after(x));  // trip 2
  if ((int)blockIdx.x * kThreads >= rows * (F / 4)) return;
  const int z = zero_after(rows);  // trip 3
  const int* perm = *reinterpret_cast<const int* const*>(base + 0x58 + z);
  const float* in = *reinterpret_cast<const float* const*>(base + 0x68 + z);
  float* out = *reinterpret_cast<float* const*>(base + 0x88 + z);
  gather(perm, in, out, rows);
}
__global__ __launch_bounds__(kThreads) void k_pinned(Args a) {
  asm volatile("" ::"s"(a.xcd), "s"(a.rows), "s"(a.perm), "s"(a.in), "s"(a.out));
  if (a.xcd > 0 && (int)(blockIdx.x % 8) >= a.xcd) return;
  if ((int)blockIdx.x * kThreads >= a.rows * (F / 4)) return;
  gather(a.perm, a.in, a.out, a.rows);
}
__global__ __launch_bounds__(kThreads) void k_preload(int xcd, int rows, const int* perm, const float* in, float* out,
                                                      Rest rest) {
  if (xcd > 0 && (int)(blockIdx.x % 8) >= xcd) return;
  if ((int)blockIdx.x * kThreads >= rows * (F / 4)) return;
  gather(perm, in, out, rows);
}
// block: [perm R ints (padded to R + 3 & ~3) | buffer 0 | buffer 1]
template <int PAR>
__global__ __launch_bounds__(kThreads) void k_pointer(float* block) {
  constexpr int P = (R + 3) & ~3;
  const int* perm = reinterpret_cast<const int*>(block);
  float* b0 = block + P;
  float* b1 = b0 + (size_t)R * F;
  gather(perm, PAR ? b1 : b0, PAR ? b0 : b1, R);
}
}  // namespace

#define KF_CHECK(e)                     \
  do {                                  \
    const hipError_t err_ = (e);        \
    if (err_ != hipSuccess) return (int)err_; \
  } while (0)

namespace {
// what a run holds on the device: released on every way out of kf_run
struct Run {
  float* block = nullptr;
  hipStream_t st = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~Run() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    if (st) (void)hipStreamDestroy(st);
    if (block) (void)hipFree(block);
  }
};
}  // namespace

extern "C" int kf_run(int variant, int n, int reps, double* us_per_launch) {
  constexpr int P = (R + 3) & ~3;
  Run run;
  float*& block = run.block;
  KF_CHECK(hipMalloc(&block, sizeof(float) * (P + 2 * (size_t)R * F)));
  {
    int* hp = new int[P];
    uint32_t s = 12345u;
    for (int i = 0; i < P; ++i) hp[i] = i < R ? i : 0;
    for (int i = R - 1; i > 0; --i) {  // Fisher-Yates with an LCG: a fixed permutation of the rows
      s = s * 1664525u + 1013904223u;
      const int k = (int)(s % (uint32_t)(i + 1));
      const int t = hp[i]; hp[i] = hp[k]; hp[k] = t;
    }
    const hipError_t e = hipMemcpy(block, hp, sizeof(int) * P, hipMemcpyHostToDevice);
    delete[] hp;
    KF_CHECK(e);
  }
  KF_CHECK(hipMemset(block + P, 0, sizeof(float) * 2 * (size_t)R * F));
  hipStream_t& st = run.st;
  KF_CHECK(hipStreamCreate(&st));
  auto launch = [&](int i) -> hipError_t {
    float* b[2] = {block + P, block + P + (size_t)R * F};
    Args a{};
    a.xcd = 0; a.perm = reinterpret_cast<const int*>(block); a.rows = R; a.in = b[i & 1]; a.out = b[(i + 1) & 1];
    switch (variant) {
      case 0: hipLaunchKernelGGL(k_lazy, dim3(kGrid), dim3(kThreads), 0, st, a); break;
      case 1: hipLaunchKernelGGL(k_pinned, dim3(kGrid), dim3(kThreads), 0, st, a); break;
      case 2: hipLaunchKernelGGL(k_preload, dim3(kGrid), dim3(kThreads), 0, st, a.xcd, a.rows, a.perm, a.in, a.out, Rest{}); break;
      default:
        if (i & 1) hipLaunchKernelGGL(k_pointer<1>, dim3(kGrid), dim3(kThreads), 0, st, block);
        else hipLaunchKernelGGL(k_pointer<0>, dim3(kGrid), dim3(kThreads), 0, st, block);
    }
    return hipGetLastError();
  };
  for (int i = 0; i < 4; ++i) KF_CHECK(launch(i));
  KF_CHECK(hipStreamSynchronize(st));
  hipGraph_t& graph = run.graph;
  hipGraphExec_t& exec = run.exec;
  KF_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < n; ++i) {
    const hipError_t e = launch(i);
    if (e != hipSuccess) {
      (void)hipStreamEndCapture(st, &graph);
      return (int)e;
    }
  }
  KF_CHECK(hipStreamEndCapture(st, &graph));
  KF_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  for (int i = 0; i < 5; ++i) KF_CHECK(hipGraphLaunch(exec, st));
  KF_CHECK(hipStreamSynchronize(st));
  hipEvent_t &e0 = run.e0, &e1 = run.e1;
  KF_CHECK(hipEventCreate(&e0));
  KF_CHECK(hipEventCreate(&e1));
  KF_CHECK(hipEventRecord(e0, st));
  for (int i = 0; i < reps; ++i) KF_CHECK(hipGraphLaunch(exec, st));
  KF_CHECK(hipEventRecord(e1, st));
  KF_CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  KF_CHECK(hipEventElapsedTime(&ms, e0, e1));
  *us_per_launch = (double)ms * 1e3 / ((double)reps * n);
  return 0;
}

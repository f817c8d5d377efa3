// gdd_runtime.hip — error state, ABI version, device check, and the hipcub-backed scan/sort
// primitives the kernels share.
#include "gdd_common.hpp"

#include <hipcub/hipcub.hpp>

#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

namespace gdd {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

size_t scan_i32_ws_bytes(int64_t n) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const int32_t*)nullptr, (int32_t*)nullptr,
                                   (int)n);
  return align256(bytes);
}

int exclusive_scan_i32(const int32_t* in, int32_t* out, int64_t n, void* ws, size_t ws_bytes,
                       hipStream_t s) {
  size_t need = 0;
  GDD_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, (int)n, s));
  if (need > ws_bytes) return fail(GDD_E_WORKSPACE, "scan workspace %zu < %zu", ws_bytes, need);
  GDD_HIP(hipcub::DeviceScan::ExclusiveSum(ws, need, in, out, (int)n, s));
  return GDD_OK;
}

size_t sort_pairs_ws_bytes(int64_t n) {
  size_t bytes = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const int32_t*)nullptr, (int32_t*)nullptr,
                                     (const int32_t*)nullptr, (int32_t*)nullptr, (int)n);
  return align256(bytes);
}

// stable LSD radix sort of (key, value) pairs on bits [0, end_bit)
int sort_pairs_i32(const int32_t* keys_in, int32_t* keys_out, const int32_t* vals_in,
                   int32_t* vals_out, int64_t n, int end_bit, void* ws, size_t ws_bytes,
                   hipStream_t s) {
  size_t need = 0;
  GDD_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, keys_in, keys_out, vals_in, vals_out,
                                             (int)n, 0, end_bit, s));
  if (need > ws_bytes) return fail(GDD_E_WORKSPACE, "sort workspace %zu < %zu", ws_bytes, need);
  GDD_HIP(hipcub::DeviceRadixSort::SortPairs(ws, need, keys_in, keys_out, vals_in, vals_out,
                                             (int)n, 0, end_bit, s));
  return GDD_OK;
}

int sort_pairs_u32(const int32_t* keys_in, int32_t* keys_out, const int32_t* vals_in,
                   int32_t* vals_out, int64_t n, void* ws, size_t ws_bytes, hipStream_t s) {
  const uint32_t* kin = reinterpret_cast<const uint32_t*>(keys_in);
  uint32_t* kout = reinterpret_cast<uint32_t*>(keys_out);
  size_t need = 0;
  GDD_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, kin, kout, vals_in, vals_out, (int)n, 0, 32, s));
  if (need > ws_bytes) return fail(GDD_E_WORKSPACE, "sort workspace %zu < %zu", ws_bytes, need);
  GDD_HIP(hipcub::DeviceRadixSort::SortPairs(ws, need, kin, kout, vals_in, vals_out, (int)n, 0, 32, s));
  return GDD_OK;
}

// ---- launch-sequence replay --------------------------------------------------------------------
namespace {
// GDD_FORCE's token `name` (or `name=value`): its value text, nullptr if absent
bool force_token(const char* name, std::string* value) {
  const char* e = getenv("GDD_FORCE");
  if (e == nullptr) return false;
  const std::string all(e), want(name);
  size_t p = 0;
  while (p <= all.size()) {
    size_t q = all.find(',', p);
    if (q == std::string::npos) q = all.size();
    const std::string tok = all.substr(p, q - p);
    const size_t eq = tok.find('=');
    if (tok.substr(0, eq) == want) {
      if (value) *value = eq == std::string::npos ? std::string() : tok.substr(eq + 1);
      return true;
    }
    p = q + 1;
  }
  return false;
}
}  // namespace

bool forced(const char* token) { return force_token(token, nullptr); }

double forced_value(const char* token, double dflt) {
  std::string v;
  if (!force_token(token, &v) || v.empty()) return dflt;
  return atof(v.c_str());
}

namespace {
struct GraphEntry {
  std::string key;  // site, device, caller key
  hipGraphExec_t exec = nullptr;
  uint64_t last_use = 0;
};
std::mutex g_graph_mu;
std::vector<GraphEntry> g_graphs;
uint64_t g_graph_tick = 0;
hipStream_t g_capture_stream[64] = {};
constexpr size_t kGraphCap = 512;

int graph_mode() {
  const char* e = getenv("GDD_GRAPH");
  return e ? atoi(e) : 0;
}
}  // namespace

int replay_or_run(const char* site, const void* key, size_t key_bytes, hipStream_t s,
                  const std::function<int(hipStream_t)>& enqueue) {
  const int mode = graph_mode();
  if (mode <= 0) return enqueue(s);
  int dev = 0;
  GDD_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return enqueue(s);
  std::string k(site);
  k.push_back('\0');
  k.append(reinterpret_cast<const char*>(&dev), sizeof(dev));
  k.append(static_cast<const char*>(key), key_bytes);
  std::lock_guard<std::mutex> lock(g_graph_mu);
  GraphEntry* e = nullptr;
  for (auto& g : g_graphs)
    if (g.key == k) {
      e = &g;
      break;
    }
  if (e && e->exec) {
    e->last_use = ++g_graph_tick;
    GDD_HIP(hipGraphLaunch(e->exec, s));
    return GDD_OK;
  }
  auto make_room = [&]() -> int {  // least recently used entry out once the cache is full
    if (g_graphs.size() < kGraphCap) return GDD_OK;
    size_t old = 0;
    for (size_t i = 1; i < g_graphs.size(); ++i)
      if (g_graphs[i].last_use < g_graphs[old].last_use) old = i;
    if (g_graphs[old].exec) {
      GDD_HIP(hipDeviceSynchronize());  // eviction is rare; never destroy a graph in flight
      GDD_HIP(hipGraphExecDestroy(g_graphs[old].exec));
    }
    g_graphs.erase(g_graphs.begin() + (long)old);
    return GDD_OK;
  };
  if (!e && mode == 1) {  // first sight: run eagerly, record on the next occurrence
    if (int rc = make_room()) return rc;
    GraphEntry ne;
    ne.key = k;
    ne.last_use = ++g_graph_tick;
    g_graphs.push_back(std::move(ne));
    return enqueue(s);
  }
  if (!g_capture_stream[dev]) GDD_HIP(hipStreamCreateWithFlags(&g_capture_stream[dev], hipStreamNonBlocking));
  hipStream_t cs = g_capture_stream[dev];
  GDD_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue(cs);
  hipGraph_t graph = nullptr;
  const hipError_t ec = hipStreamEndCapture(cs, &graph);
  if (rc) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  if (ec != hipSuccess) return fail((int)ec, "%s: graph capture failed: %s", site, hipGetErrorString(ec));
  hipGraphExec_t exec = nullptr;
  const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ei != hipSuccess) return fail((int)ei, "%s: graph instantiate failed: %s", site, hipGetErrorString(ei));
  if (!e) {
    if (int rc2 = make_room()) return rc2;
    g_graphs.emplace_back();
    e = &g_graphs.back();
    e->key = k;
  }
  e->exec = exec;
  e->last_use = ++g_graph_tick;
  GDD_HIP(hipGraphLaunch(exec, s));
  return GDD_OK;
}

// streaming copy used to measure the achievable HBM bandwidth on the box (report the
// measured copy peak beside the 8 TB/s spec). Grid-stride over 16-byte words, 4 in flight per lane,
// nontemporal: the fastest of the shapes tools/probe/copy_probe.hip compares (~6.1 TB/s on 1 GiB).
typedef float v4f __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_stream_copy(const v4f* __restrict__ src,
                                                     v4f* __restrict__ dst, int64_t n16) {
  const int64_t step = (int64_t)gridDim.x * 1024;
  for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x; i < n16; i += step) {
    v4f v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = i + u * 256;
      if (j < n16) v[u] = __builtin_nontemporal_load(src + j);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = i + u * 256;
      if (j < n16) __builtin_nontemporal_store(v[u], dst + j);
    }
  }
}

}  // namespace gdd

extern "C" {

int gdd_stream_copy(const void* src, void* dst, size_t bytes, gdd_stream_t stream) {
  GDD_REQUIRE(src && dst && bytes % 16 == 0, "stream_copy: 16-byte multiple and non-null buffers");
  GDD_REQUIRE(((uintptr_t)src | (uintptr_t)dst) % 16 == 0, "stream_copy: 16-byte aligned buffers");
  const int64_t n16 = (int64_t)(bytes / 16);
  if (n16 == 0) return GDD_OK;
  const int64_t want = (n16 + 1023) / 1024;
  const unsigned g = (unsigned)(want < 8192 ? want : 8192);
  gdd::k_stream_copy<<<g, 256, 0, gdd::to_hip(stream)>>>(static_cast<const gdd::v4f*>(src),
                                                        static_cast<gdd::v4f*>(dst), n16);
  GDD_LAUNCHED();
  return GDD_OK;
}

const char* gdd_last_error(void) { return gdd::g_last_error.c_str(); }

int gdd_abi_version(void) { return 3; }

int gdd_spin_limit(void) { return gdd::kSpinLimit; }

int gdd_device_ok(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
  return std::string(prop.gcnArchName).rfind("gfx950", 0) == 0 ? 1 : 0;
}

}  // extern "C"

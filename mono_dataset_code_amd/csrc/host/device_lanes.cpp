#include "device_lanes.h"

#include <dlfcn.h>
#include <sched.h>
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "MdcBind.h"
#include "host_device.h"
#include "mdc_hip.h"
#include "sibling_library.h"

namespace mdc_host {

bool DeviceLanes::load_multi() {
  if (mapi_.lib) return true;
  void* lib = open_sibling_library("libmdc_multi.so");  // RCCL keeps static state and helper threads: never unmapped again
  if (!lib) return false;
  mapi_.create = (int (*)(const int*, int, void**))dlsym(lib, "mdc_multi_create");
  mapi_.destroy = (void (*)(void*))dlsym(lib, "mdc_multi_destroy");
  mapi_.ctx = (mdc_ctx * (*)(void*, int)) dlsym(lib, "mdc_multi_ctx");
  mapi_.bcast = (int (*)(void*, int))dlsym(lib, "mdc_multi_bcast_tables");
  mapi_.last_error = (const char* (*)(const void*))dlsym(lib, "mdc_multi_last_error");
  if (!mapi_.create || !mapi_.destroy || !mapi_.ctx || !mapi_.bcast || !mapi_.last_error) {
    dlclose(lib);
    return false;
  }
  mapi_.lib = lib;
  return true;
}

static const PngdApi* load_pngd(const char* env, const char* file, const char* prefix) {
  void* lib = open_sibling_library(file, env);  // holds a HIP module: never unmapped again
  if (!lib) return 0;
  const std::string pre(prefix);
  PngdApi* a = new PngdApi;  // one per library and process, never freed
  a->create = (int (*)(int, int, int, int, void**))dlsym(lib, (pre + "create").c_str());
  a->destroy = (void (*)(void*))dlsym(lib, (pre + "destroy").c_str());
  a->decode_host = (int (*)(void*, const void* const*, const long long*, int, int*, const unsigned char**))dlsym(lib, (pre + "decode_host").c_str());
  a->last_error = (const char* (*)())dlsym(lib, (pre + "last_error").c_str());
  a->stream = (void* (*)(void*))dlsym(lib, (pre + "stream").c_str());
  a->synchronize = (int (*)(void*))dlsym(lib, (pre + "synchronize").c_str());
  return a->create && a->destroy && a->decode_host && a->last_error && a->stream && a->synchronize ? a : 0;
}

const PngdApi* pngd_api(bool parallel_matches) {
  if (parallel_matches) {
    static const PngdApi* apix = load_pngd("MDC_LIB_PNGDX", "libmdc_pngdx.so", "mdcx_");
    return apix;
  }
  static const PngdApi* api = load_pngd("MDC_LIB_PNGD", "libmdc_pngd.so", "mdci_");
  return api;
}

// MDC_DEVICES: "all" or "0,1,..." (unset or empty: no list)
static std::vector<int> device_list() {
  std::vector<int> devs;
  const char* e = std::getenv("MDC_DEVICES");
  if (!e || !*e) return devs;
  if (std::string(e) == "all") {
    const int n = mdc_device_count();
    for (int i = 0; i < n; i++) devs.push_back(i);
    return devs;
  }
  for (const char* p = e; *p;) {
    char* end = 0;
    const long v = std::strtol(p, &end, 10);
    if (end == p) break;
    if (v >= 0) devs.push_back((int)v);
    p = *end == ',' ? end + 1 : end;
    if (*end && *end != ',') break;
  }
  return devs;
}

void DeviceLanes::add_lane(mdc_ctx* gpu, int device, bool twin) {
  Lane ln;
  ln.gpu = gpu;
  ln.device = device;
  ln.twin = twin;
  lanes.push_back(ln);
}

// `c` with the tables bound, or nothing: a context that cannot take them is destroyed (*why: the library's words)
mdc_ctx* DeviceLanes::bind_tables(mdc_ctx* c, std::string* why) {
  if (c && mdc_bind_objects(c, fov_, photo_) == MDC_OK) return c;
  *why = mdc_last_error(c);
  if (c) mdc_destroy(c);
  return 0;
}

// A context on device `device` with the tables bound, or nothing
mdc_ctx* DeviceLanes::bound_context(int device, std::string* why) {
  mdc_ctx* c = 0;
  if (mdc_create(device, &c) == MDC_OK) return bind_tables(c, why);
  *why = mdc_last_error(c);
  if (c) mdc_destroy(c);
  return 0;
}

mdc_ctx* DeviceLanes::open(const UndistorterFOV* fov, const PhotometricUndistorter* photo) {
  fov_ = fov;
  photo_ = photo;
  const std::vector<int> devs = device_list();
  bool distinct = devs.size() > 1;
  for (size_t i = 0; i < devs.size(); i++)
    for (size_t j = i + 1; j < devs.size(); j++)
      if (devs[i] == devs[j]) distinct = false;
  // (MDC_READER_FORCE_RCCL=1: take the RCCL path for a single listed device too -- a world of one --, so that a one-GPU box
  // executes the dlopen, the communicator set-up, the broadcast and the lanes on libmdc_multi's contexts)
  const bool force_rccl = std::getenv("MDC_READER_FORCE_RCCL") != 0 && devs.size() == 1;
  if ((distinct || force_rccl) && load_multi()) {  // one RCCL broadcast of rank 0's tables
    void* m = 0;
    if (mapi_.create(devs.data(), (int)devs.size(), &m) == MDC_OK && m) {
      mdc_ctx* root = mapi_.ctx(m, 0);
      if (root && mdc_bind_objects(root, fov, photo) == MDC_OK && mapi_.bcast(m, 0) == MDC_OK) {
        multi_ = m;
        for (size_t r = 0; r < devs.size(); r++) add_lane(mapi_.ctx(m, (int)r), devs[r]);
        std::printf("DatasetReader: %d devices, calibration tables broadcast over RCCL\n", (int)devs.size());
        return lanes[0].gpu;
      }
      std::fprintf(stderr, "DatasetReader: RCCL table broadcast failed (%s); every device takes the tables from the host\n", mapi_.last_error(m));
      mapi_.destroy(m);
    }
  }
  std::string why;
  if (devs.size() > 1) {
    for (size_t r = 0; r < devs.size(); r++) {
      if (mdc_ctx* c = bound_context(devs[r], &why)) add_lane(c, devs[r]);
      else std::fprintf(stderr, "DatasetReader: device %d: %s; not used\n", devs[r], why.c_str());
    }
    if (!lanes.empty()) {
      std::printf("DatasetReader: %d devices, calibration tables uploaded to each\n", (int)lanes.size());
      return lanes[0].gpu;
    }
  }
  mdc_ctx* gpu = devs.size() == 1 ? 0 : open_device_context("DatasetReader");
  if (devs.size() == 1 && mdc_create(devs[0], &gpu) != MDC_OK) {
    std::fprintf(stderr, "DatasetReader: no GPU context on device %d (%s)\n", devs[0], mdc_last_error(0));
    gpu = 0;
  }
  if (gpu && !(gpu = bind_tables(gpu, &why))) std::fprintf(stderr, "DatasetReader: table upload failed: %s\n", why.c_str());
  mdc_info inf;
  add_lane(gpu, (gpu && mdc_get_info(gpu, &inf) == MDC_OK) ? inf.device : -1);
  return gpu;
}

// getImagesDevice: its results cross no bus on the way out, so what limits one pipelined call is its own fill and drain (upload of
// the first chunk, fused pass of the last).  Two calls from two host threads on two contexts of the SAME device overlap them:
// measured on a zipped 1280x1024 JPEG sequence 99.6 k frames/s with one lane, 126 k with two lanes and 128-frame chunks, 109 k with
// three (profiles/r05_reader_device_rates.txt).  The twin is made at the first getImagesDevice call (MDC_DEVICE_LANES=1: never).
void DeviceLanes::ensure_device_lanes() {
  static const int want = [] {
    const char* e = std::getenv("MDC_DEVICE_LANES");
    return e ? std::max(1, std::min(4, std::atoi(e))) : 2;
  }();
  if (lanes.empty() || !lanes[0].gpu) return;
  int have = 0;
  for (const Lane& ln : lanes) have += ln.device == lanes[0].device && ln.gpu ? 1 : 0;
  bool made = false;
  std::string why;
  for (; have < want; have++) {
    mdc_ctx* c = bound_context(lanes[0].device, &why);
    if (!c) return;  // one lane does the work
    add_lane(c, lanes[0].device, true);
    made = true;
  }
  // with a second call to hide a chunk's fill and drain behind, longer chunks win (Huffman: 5.3 us per frame at 128, 6.7 at 64).  Given ONCE,
  // when a twin was made, and as a hint: a caller's own MDC_OPT_DEVICE_PIPELINE_CHUNK on the public context (getContext()) and
  // MDC_PIPE_DEV_CHUNK in the environment both stay in force
  if (made && have >= 2)
    for (Lane& ln : lanes)
      if (ln.device == lanes[0].device && ln.gpu) (void)mdc_set_option(ln.gpu, MDC_OPT_DEVICE_PIPELINE_CHUNK_HINT, 128);
}

// device outputs live on ONE device, the first lane's: the lanes on that device take part (MDC_DEVICES=0,0: two lanes on one GPU --
// two host threads whose pipelined calls overlap, one lane's fill and drain under the other's decode)
std::vector<Lane*> DeviceLanes::for_batch(bool device_outputs) {
  if (!host_lanes) host_lanes = (int)lanes.size();
  std::vector<Lane*> use;
  if (device_outputs) {
    ensure_device_lanes();
    for (Lane& ln : lanes)
      if (ln.device == lanes[0].device && ln.gpu) use.push_back(&ln);
  } else {
    for (int l = 0; l < host_lanes; l++) use.push_back(&lanes[(size_t)l]);  // (twin lanes made for getImagesDevice take no part in getImages)
  }
  return use;
}

void DeviceLanes::close() {
  for (Lane& ln : lanes) {
    ln.ring_block.release();
    if (ln.pngd && ln.pngd_from) ln.pngd_from->destroy(ln.pngd);
    ln.pngd = 0;
    if ((!multi_ || ln.twin) && ln.gpu) mdc_destroy(ln.gpu);
  }
  if (multi_) mapi_.destroy(multi_);
  multi_ = 0;
  lanes.clear();
  // (no dlclose: libmdc_multi.so pulls in librccl, whose static state and helper threads must outlive this reader -- unloading it
  // mid-process risks a crash at exit or when the next reader loads it again; the handle is RTLD_NODELETE and simply dropped)
  mapi_.lib = 0;
}

// A lane's host thread issues its device's copies and launches: it belongs on the CPUs next to that GPU (on a two-socket 8-GPU node
// half of the devices hang off the other socket; a thread there pays the socket hop on every doorbell and staging copy).
// /sys/bus/pci/devices/<pci>/local_cpulist ("0-63,128-191") -> sched_setaffinity of the calling thread.  MDC_NUMA_PIN=0 turns it off;
// any failure (no sysfs, empty list, a cpuset that excludes those CPUs) leaves the thread where it is.
static std::vector<int> parse_cpulist(const std::string& text) {
  std::vector<int> cpus;
  size_t i = 0;
  while (i < text.size()) {
    while (i < text.size() && !isdigit((unsigned char)text[i])) i++;
    if (i >= text.size()) break;
    int a = 0, b;
    while (i < text.size() && isdigit((unsigned char)text[i])) a = a * 10 + (text[i++] - '0');
    b = a;
    if (i < text.size() && text[i] == '-') {
      i++;
      b = 0;
      while (i < text.size() && isdigit((unsigned char)text[i])) b = b * 10 + (text[i++] - '0');
    }
    for (int c = a; c <= b && c < CPU_SETSIZE && cpus.size() < 4096; c++) cpus.push_back(c);
  }
  return cpus;
}
void pin_thread_near_device(mdc_ctx* gpu) {
  static const bool enabled = [] {
    const char* e = std::getenv("MDC_NUMA_PIN");
    return !e || std::atoi(e) != 0;
  }();
  char pci[32];
  if (!enabled || !gpu || mdc_device_pci_bus_id(gpu, pci, sizeof pci) != MDC_OK) return;
  std::ifstream f(std::string("/sys/bus/pci/devices/") + pci + "/local_cpulist");
  std::string line;
  if (!f || !std::getline(f, line)) return;
  const std::vector<int> cpus = parse_cpulist(line);
  if (cpus.empty()) return;
  cpu_set_t set;
  CPU_ZERO(&set);
  for (int c : cpus) CPU_SET(c, &set);
  (void)sched_setaffinity(0, sizeof set, &set);  // refused (cpuset): stay
}

}  // namespace mdc_host

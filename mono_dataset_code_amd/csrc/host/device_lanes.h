// The devices a reader works on.  Frames of a sequence are independent (reference src/BenchmarkDatasetReader.h:188-243), so getImages
// deals its range to every device listed in MDC_DEVICES in chunks (lane l takes chunks l, l + L, ...).  All lanes hold the SAME tables: with
// libmdc_multi.so next to this library and distinct devices, rank 0's tables go out in one RCCL broadcast over xGMI
// (mdc_multi_bcast_tables); otherwise (the library is missing, or a device is listed twice -- a test on a one-GPU box) every
// context takes them from the host objects directly.  Either way the bytes are the host's.
#pragma once
#include <vector>

#include "decode_pool.h"

struct mdc_ctx;
class UndistorterFOV;
class PhotometricUndistorter;

namespace mdc_host {

// One lane per device the reader may use (MDC_DEVICES; lanes[0] holds the reader's public context): its context and its own decode
// ring -- ONE page-locked block, slot i at ring_block.p + i * ring_stride (a chunk's uploads are then one strided copy instead of
// one copy per frame), ring_bytes per buffer (a frame, or a record when the GPU JPEG stage is on).
// libmdc_pngd.so (include/mdc_pngd.h), loaded at run time: the device PNG decoder of getImagesDevice
struct PngdApi {
  int (*create)(int, int, int, int, void**) = 0;
  void (*destroy)(void*) = 0;
  int (*decode_host)(void*, const void* const*, const long long*, int, int*, const unsigned char**) = 0;
  const char* (*last_error)() = 0;
  void* (*stream)(void*) = 0;
  int (*synchronize)(void*) = 0;
};
// The library next to this one (or the file MDC_LIB_PNGD names), opened once per process and never closed; 0 when it is not there:
// PNG frames then take the host decoder, silently.  parallel_matches: libmdc_pngdx.so (include/mdc_pngdx.h; MDC_LIB_PNGDX), the same
// interface under mdcx_ names, by the same rules.
const PngdApi* pngd_api(bool parallel_matches = false);

struct Lane {
  void* pngd = 0;  // the lane's mdci_decoder (or mdcx_decoder), made at first use for pngd_frames frames of the reader's size
  const PngdApi* pngd_from = 0;  // the library that made it
  int pngd_frames = 0;
  long png_frames = 0;  // statistics: frames it decoded
  mdc_ctx* gpu = 0;
  int device = -1;
  bool twin = false;  // a second context on lane 0's device, made for getImagesDevice (ensure_device_lanes); owned by the reader
  HostBuffer ring_block;
  size_t ring_stride = 0, ring_bytes = 0;
  int ring_slots = 0;
  long frames = 0;  // statistics over the reader's life: frames produced, seconds waiting for the decoders / inside GPU calls
  double t_wait = 0, t_gpu = 0;
};

class DeviceLanes {
 public:
  std::vector<Lane> lanes;
  int host_lanes = 0;  // lanes getImages deals its range to (what open() made); 0 until the first batch call

  // One context per device of MDC_DEVICES (unset: the one device of $MDC_DEVICE / the calling thread) holding BOTH objects'
  // tables; says on stdout / stderr what it did.  Returns lane 0's context (0: no GPU).
  mdc_ctx* open(const UndistorterFOV* fov, const PhotometricUndistorter* photo);
  void close();
  // The lanes of a getImages call, or (device_outputs) of a getImagesDevice call: those on lane 0's device, twins included
  std::vector<Lane*> for_batch(bool device_outputs);
  int device_count() const { return host_lanes ? host_lanes : (int)lanes.size(); }

 private:
  struct MultiApi {
    void* lib = 0;
    int (*create)(const int*, int, void**) = 0;
    void (*destroy)(void*) = 0;
    mdc_ctx* (*ctx)(void*, int) = 0;
    int (*bcast)(void*, int) = 0;
    const char* (*last_error)(const void*) = 0;
  } mapi_;
  bool load_multi();
  void add_lane(mdc_ctx* gpu, int device, bool twin = false);
  mdc_ctx* bind_tables(mdc_ctx* c, std::string* why);
  mdc_ctx* bound_context(int device, std::string* why);
  void ensure_device_lanes();
  const UndistorterFOV* fov_ = 0;
  const PhotometricUndistorter* photo_ = 0;
  void* multi_ = 0;  // libmdc_multi.so's object when the lanes' contexts are its (RCCL table broadcast), else the lanes own theirs
};

// Moves the calling thread to the CPUs next to the context's GPU (MDC_NUMA_PIN=0: never)
void pin_thread_near_device(mdc_ctx* gpu);

}  // namespace mdc_host

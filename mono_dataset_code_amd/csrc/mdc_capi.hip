// libmdc_hip.so -- the context behind the C ABI in include/mdc_hip.h: the last error, lifetime, options and info, the device
// copies of the calibration tables with their setters and their blob, flag normalisation exactly as
// src/PhotometricUndistorter.cpp:173-189 (reference repo), mdc_synchronize.  What runs on the frames is in the other units
// (file map: mdc_ctx.h).  There is NO CPU implementation of the per-frame maths in this library: without a HIP device every
// entry point fails with MDC_ERR_NO_DEVICE.
#include "mdc_ctx.h"

using namespace mdc;

namespace mdc {

static thread_local std::string g_create_err;
// mdc_last_error(ctx) returns the calling thread's own last failure on that context if it had one (several threads may
// use one context), else the context's most recent one
static thread_local std::string t_err, t_err_other;
static thread_local const mdc_ctx* t_err_ctx = nullptr;

int fail(mdc_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) {
    {
      std::lock_guard<std::mutex> lk(c->err_mu);
      c->err = buf;
    }
    t_err = buf;
    t_err_ctx = c;
  } else {
    g_create_err = buf;
  }
  return code;
}

// The reference's flag degradation, src/PhotometricUndistorter.cpp:173-189.
void normalise(const mdc_ctx* c, unsigned flags, bool& g, bool& v, bool& o) {
  g = (flags & MDC_GAMMA) != 0;
  v = (flags & MDC_VIGNETTE) != 0;
  o = (flags & MDC_KILL_OVEREXPOSED) != 0;
  if (!c->valid_gamma && g) g = false;
  if (!c->valid_vignette && v) v = false;
  if (!g && v) {
    v = false;
    g = false;
  }
}

const float* lut_for(const mdc_ctx* c, bool g, bool o) { return c->d_luts + 256 * ((g ? 1 : 0) | (o ? 2 : 0)); }

int upload_luts(mdc_ctx* c) {
  std::vector<float> l(4 * 256);
  for (int var = 0; var < 4; var++)
    for (int b = 0; b < 256; b++) {
      float x = (var & 1) ? (c->valid_gamma ? c->h_ginv[b] : (float)b) : (float)b;
      if ((var & 2) && b == 255) x = std::numeric_limits<float>::quiet_NaN();
      l[var * 256 + b] = x;
    }
  if (!c->d_luts) MDC_HIP(c, hipMalloc(&c->d_luts, l.size() * sizeof(float)));
  MDC_HIP(c, hipMemcpy(c->d_luts, l.data(), l.size() * sizeof(float), hipMemcpyHostToDevice));
  return MDC_OK;
}

struct BlobHeader {
  uint32_t magic, version;
  int32_t in_w, in_h, rm_in_w, rm_in_h, out_w, out_h;
  int32_t valid_gamma, valid_vignette, valid_remap, pad;
};
constexpr uint32_t kMagic = 0x4d444331u;  // "MDC1"

}  // namespace mdc

static int set_photometric_locked(mdc_ctx* c, const float* ginv, const float* vignette_inv, int w, int h);
static int set_remap_locked(mdc_ctx* c, const float* rx, const float* ry, int in_w, int in_h, int out_w, int out_h);

extern "C" {

int mdc_create(int device, mdc_ctx** out) try {
  if (!out) return fail(nullptr, MDC_ERR_ARG, "mdc_create: out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, MDC_ERR_NO_DEVICE, "no HIP device visible (%s); this library has no CPU fallback",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device == -1 && hipGetDevice(&device) != hipSuccess) device = 0;
  if (device < 0 || device >= n) return fail(nullptr, MDC_ERR_ARG, "device %d out of range [0,%d)", device, n);
  mdc_ctx* c = new mdc_ctx();
  c->device = device;
  DeviceGuard dg(device);
  c->h_ginv.assign(256, 0.f);
  if (const char* e = getenv("MDC_PIN_CALLER_BUFFERS")) c->opt_pin_caller = atoi(e) != 0;
  if (const char* e = getenv("MDC_ZERO_COPY")) c->opt_zero_copy = std::max(0, std::min(2, atoi(e)));  // as MDC_OPT_ZERO_COPY, for callers that cannot be recompiled
  int rc = upload_luts(c);
  if (rc == MDC_OK && hipMalloc(&c->d_vcal_max, mdc_ctx::kVcalMaxWords * sizeof(unsigned)) != hipSuccess)
    rc = fail(c, MDC_ERR_HIP, "hipMalloc of the context's scratch words failed");
  if (rc != MDC_OK) {
    g_create_err = t_err;
    if (c->d_luts) (void)hipFree(c->d_luts);
    t_err_ctx = nullptr;
    delete c;
    return rc;
  }
  *out = c;
  return MDC_OK;
} MDC_CATCH(nullptr)

void mdc_destroy(mdc_ctx* c) {
  if (!c) return;
  {
    DeviceGuard dg(c->device);
    for (mdc_ctx::HostSlot* h : c->slots) {
      if (h->stream) (void)hipStreamSynchronize(h->stream);
      if (h->d_in) (void)hipFree(h->d_in);
      if (h->d_out) (void)hipFree(h->d_out);
      if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
      if (h->ev_join) (void)hipEventDestroy(h->ev_join);
      if (h->stream) (void)hipStreamDestroy(h->stream);
      delete h;
    }
    c->slots.clear();
    for (int k = 0; k < 2; k++)
      if (c->pipe_stream[k]) (void)hipStreamSynchronize(c->pipe_stream[k]);
    if (c->pipe_up_stream) (void)hipStreamSynchronize(c->pipe_up_stream);
    unpin_all(c);
    free_plan(c);
    {  // striped buffers of mdc_device_alloc the caller never gave back: their arenas cannot be reached without the context
      std::vector<void*> arenas;
      {
        std::lock_guard<std::mutex> lk(c->striped_mu);
        for (auto& kv : c->striped) arenas.push_back(kv.second);
        c->striped.clear();
      }
      for (void* a : arenas) {
        mdc_striped_set set;
        memset(&set, 0, sizeof set);
        set.handle = a;
        (void)mdc_free_striped_set_device(c, &set);
      }
    }
    void* ptrs[] = {c->d_luts, c->d_vinv, c->d_rx, c->d_ry, c->d_vcal_max, c->d_pipe_in[0], c->d_pipe_in[1], c->d_pipe_out[0], c->d_pipe_out[1],
                    c->d_pipe_rec[0], c->d_pipe_rec[1], c->d_pipe_strm[0], c->d_pipe_strm[1], c->d_pipe_status[0], c->d_pipe_status[1], c->d_pipe_seg[0], c->d_pipe_seg[1]};
    for (void* p : ptrs)
      if (p) (void)hipFree(p);
    if (c->h_pipe_status) (void)hipHostFree(c->h_pipe_status);
    for (int k = 0; k < 2; k++) {
      if (c->pipe_done[k]) (void)hipEventDestroy(c->pipe_done[k]);
      if (c->pipe_dec[k]) (void)hipEventDestroy(c->pipe_dec[k]);
      if (c->pipe_up[k]) (void)hipEventDestroy(c->pipe_up[k]);
      if (c->pipe_huff[k]) (void)hipEventDestroy(c->pipe_huff[k]);
      if (c->pipe_stream[k]) (void)hipStreamDestroy(c->pipe_stream[k]);
    }
    if (c->pipe_up_stream) (void)hipStreamDestroy(c->pipe_up_stream);
  }
  if (t_err_ctx == c) t_err_ctx = nullptr;
  delete c;
}

const char* mdc_build_flags(void) { return mdc::build_flags_string(); }

int mdc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

const char* mdc_last_error(const mdc_ctx* c) {
  if (!c) return g_create_err.c_str();
  if (t_err_ctx == c) return t_err.c_str();
  std::lock_guard<std::mutex> lk(c->err_mu);
  t_err_other = c->err;
  return t_err_other.c_str();
}

int mdc_device_pci_bus_id(mdc_ctx* c, char* buf, size_t cap) try {
  if (!c) return MDC_ERR_ARG;
  if (!buf || cap < 13) return fail(c, MDC_ERR_ARG, "mdc_device_pci_bus_id: buffer of >= 13 bytes expected");
  char tmp[64] = {0};
  MDC_HIP(c, hipDeviceGetPCIBusId(tmp, (int)sizeof tmp, c->device));
  for (char* q = tmp; *q; q++) *q = (char)tolower((unsigned char)*q);  // sysfs spells the address in lower case
  snprintf(buf, cap, "%s", tmp);
  return MDC_OK;
} MDC_CATCH(c)

int mdc_set_option(mdc_ctx* c, int option, int value) try {
  if (!c) return MDC_ERR_ARG;
  WriteLock lk(c->mu);
  switch (option) {
    case MDC_OPT_KERNEL:
      if (value < MDC_KERNEL_AUTO || value > MDC_KERNEL_TILED) return fail(c, MDC_ERR_ARG, "bad kernel selector %d", value);
      c->opt_kernel = value;
      return MDC_OK;
    case MDC_OPT_FRAMES_PER_BLOCK:
      if (value < 0) return fail(c, MDC_ERR_ARG, "bad frames-per-block %d", value);
      c->opt_fpb = value;
      return MDC_OK;
    case MDC_OPT_TILE_ROWS: {
      if (value != 0 && value != 16 && value != 32 && value != 60 && value != 64)
        return fail(c, MDC_ERR_ARG, "tile rows must be 0 (automatic), 16, 32, 60 or 64");
      if (value == c->opt_tile_h) return MDC_OK;
      c->opt_tile_h = value;
      c->tuned_fpb = 0;  // a measured frames-per-workgroup belongs to the plan it was measured on
      if (!c->valid_remap) return MDC_OK;
      DeviceGuard dg(c->device);
      MDC_HIP(c, hipDeviceSynchronize());
      return plan_tiles(c);
    }
    case MDC_OPT_TILE_COLS: {
      if (value != 0 && value != 64 && value != 128) return fail(c, MDC_ERR_ARG, "tile columns must be 0 (automatic), 64 or 128");
      if (value == c->opt_tile_w) return MDC_OK;
      c->opt_tile_w = value;
      c->tuned_fpb = 0;
      if (!c->valid_remap) return MDC_OK;
      DeviceGuard dg(c->device);
      MDC_HIP(c, hipDeviceSynchronize());
      return plan_tiles(c);
    }
    case MDC_OPT_FRAME_INTERLEAVE:
      c->opt_interleave = value != 0;
      return MDC_OK;
    case MDC_OPT_PIN_CALLER_BUFFERS: {
      c->opt_pin_caller = value != 0;
      if (!c->opt_pin_caller) {
        DeviceGuard dg(c->device);
        MDC_HIP(c, hipDeviceSynchronize());
        unpin_all(c);
      }
      return MDC_OK;
    }
    case MDC_OPT_WINDOW_BUFFERS: {
      if (value < 0 || value > 4) return fail(c, MDC_ERR_ARG, "window buffers must be 0 (auto) or 1..4 (1: strip kernel only)");
      if (value == c->opt_nbuf) return MDC_OK;
      c->opt_nbuf = value;
      if (!c->valid_remap) return MDC_OK;
      DeviceGuard dg(c->device);
      MDC_HIP(c, hipDeviceSynchronize());
      return plan_tiles(c);
    }
    case MDC_OPT_DEVICE_PIPELINE_CHUNK:
      if (value != 0 && (value < 16 || value > 256)) return fail(c, MDC_ERR_ARG, "device pipeline chunk must be 0 (automatic) or 16..256 frames");
      c->opt_dev_chunk = value;
      return MDC_OK;
    case MDC_OPT_DEVICE_PIPELINE_CHUNK_HINT:
      if (value != 0 && (value < 16 || value > 256)) return fail(c, MDC_ERR_ARG, "device pipeline chunk hint must be 0 (none) or 16..256 frames");
      c->opt_dev_chunk_hint = value;
      return MDC_OK;
    case MDC_OPT_TAIL_TAPER:
      if (value < 0 || value > 2) return fail(c, MDC_ERR_ARG, "tail taper selector must be 0 (automatic), 1 (on) or 2 (off)");
      c->opt_taper = value;
      return MDC_OK;
    case MDC_OPT_ZERO_COPY:
      if (value < 0 || value > 2) return fail(c, MDC_ERR_ARG, "zero-copy selector must be 0 (automatic), 1 (on) or 2 (off)");
      c->opt_zero_copy = value;
      return MDC_OK;
    case MDC_OPT_PREFETCH_STREAMS:
      if (value < 0 || value > 2) return fail(c, MDC_ERR_ARG, "prefetch streams must be 0 (automatic), 1 or 2");
      c->opt_prefetch_streams = value;
      return MDC_OK;
    case MDC_OPT_PREFETCH_CHUNK:
      if (value < -1) return fail(c, MDC_ERR_ARG, "prefetch chunk must be -1 (off), 0 (automatic) or a frame count");
      c->opt_prefetch_chunk = value;
      return MDC_OK;
    case MDC_OPT_TWO_STAGE: {
      if (value < 0 || value > 2) return fail(c, MDC_ERR_ARG, "two-stage selector must be 0 (automatic), 1 (on) or 2 (off)");
      if (value == c->opt_two_stage) return MDC_OK;
      c->opt_two_stage = value;
      c->tuned_fpb = 0;
      if (!c->valid_remap) return MDC_OK;
      DeviceGuard dg(c->device);
      MDC_HIP(c, hipDeviceSynchronize());
      return plan_tiles(c);
    }
    case MDC_OPT_TILE_ORDER: {
      if (value < MDC_ORDER_BANDS || value > MDC_ORDER_BLOCKS2D) return fail(c, MDC_ERR_ARG, "bad tile order %d", value);
      if (value == c->opt_order) return MDC_OK;
      c->opt_order = value;
      if (!c->valid_remap) return MDC_OK;
      DeviceGuard dg(c->device);
      MDC_HIP(c, hipDeviceSynchronize());
      return plan_tiles(c);
    }
    case MDC_OPT_XCD_ROTATE: {
      if (value < 0 || value > 2) return fail(c, MDC_ERR_ARG, "XCD rotation must be 0 (off), 1 (on) or 2 (on, strip kernel included)");
      if (value == c->opt_xcd_rotate) return MDC_OK;
      c->opt_xcd_rotate = value;
      c->tuned_fpb = 0;
      if (!c->valid_remap) return MDC_OK;
      DeviceGuard dg(c->device);
      MDC_HIP(c, hipDeviceSynchronize());
      return plan_tiles(c);
    }
  }
  return fail(c, MDC_ERR_ARG, "unknown option %d", option);
} MDC_CATCH(c)

int mdc_get_info(mdc_ctx* c, mdc_info* i) try {
  if (!c || !i) return MDC_ERR_ARG;
  ReadLock lk(c->mu);
  memset(i, 0, sizeof *i);
  i->device = c->device;
  i->in_w = c->in_w ? c->in_w : c->rm_in_w;
  i->in_h = c->in_h ? c->in_h : c->rm_in_h;
  i->out_w = c->valid_remap ? c->out_w : 0;
  i->out_h = c->valid_remap ? c->out_h : 0;
  i->valid_gamma = c->valid_gamma;
  i->valid_vignette = c->valid_vignette;
  i->valid_remap = c->valid_remap;
  const mdc_ctx::SrcPlan& p0 = c->plan[0];
  i->tiled = c->valid_remap && p0.tiled;
  i->tile_w = p0.tiled ? p0.tile_w : c->opt_tile_w;
  i->tile_h = p0.tiled ? p0.tile_h : c->opt_tile_h;
  i->n_tiles = p0.n_tiles;
  i->lds_bytes = p0.tiled ? (int)tiled_lds_bytes(p0.win_bytes, p0.nbuf, true) : 0;
  i->two_stage = c->strip.planned ? 1 : 0;
  i->prefetch_chunk = (c->strip.planned && c->opt_prefetch_chunk >= 0 && prefetch_box_bytes(c) >= 4096) ? (int)prefetch_chunk_frames(c) : 0;
  i->prefetch_streams = i->prefetch_chunk ? prefetch_streams(c) : 0;
  if (c->strip.planned) {
    i->tiled = c->valid_remap;
    i->tile_w = kStripTileW;
    i->tile_h = kStripTileH;
    i->n_tiles = c->strip.n_tiles;
    i->lds_bytes = (int)strip_lds_bytes(c->strip.win_bytes, c->strip.nbuf, kStripWaves);
    i->window_buffers = c->strip.nbuf;
  }
  i->window_buffers = p0.tiled ? p0.nbuf : 0;
  i->f32_tiled = c->valid_remap && c->plan[1].tiled;
  i->f32_tile_w = c->plan[1].tiled ? c->plan[1].tile_w : 0;
  i->f32_tile_h = c->plan[1].tiled ? c->plan[1].tile_h : 0;
  for (int k = 0; k < 4; k++) i->src_bbox[k] = c->bbox[k];
  i->src_bbox_bytes = c->bbox[2] >= 0 ? (int64_t)(c->bbox[2] - c->bbox[0] + 1) * (c->bbox[3] - c->bbox[1] + 1) : 0;
  i->src_staged_bytes = c->strip.planned ? c->strip.staged_bytes : p0.staged_bytes;
  i->n_black = c->n_black;
  return MDC_OK;
} MDC_CATCH(c)

int mdc_set_photometric(mdc_ctx* c, const float* ginv, const float* vignette_inv, int w, int h) try {
  if (!c) return MDC_ERR_ARG;
  if (w <= 0 || h <= 0) return fail(c, MDC_ERR_ARG, "bad frame size %dx%d", w, h);
  WriteLock lk(c->mu);
  return set_photometric_locked(c, ginv, vignette_inv, w, h);
} MDC_CATCH(c)

// (lock held) The tables are replaced in place: every kernel that may still read them -- also those the
// *_device entry points put on caller streams -- has to be done first, hence the device-wide wait.
static int set_photometric_locked(mdc_ctx* c, const float* ginv, const float* vignette_inv, int w, int h) {
  DeviceGuard dg(c->device);
  MDC_HIP(c, hipDeviceSynchronize());
  c->in_w = w;
  c->in_h = h;
  c->valid_gamma = ginv != nullptr;
  if (ginv) c->h_ginv.assign(ginv, ginv + 256);
  int rc = upload_luts(c);
  if (rc != MDC_OK) return rc;
  c->valid_vignette = vignette_inv != nullptr;
  if (c->d_vinv) {
    (void)hipFree(c->d_vinv);
    c->d_vinv = nullptr;
  }
  c->h_vinv.clear();
  if (vignette_inv) {
    const size_t n = (size_t)w * h;
    c->h_vinv.assign(vignette_inv, vignette_inv + n);
    MDC_HIP(c, hipMalloc(&c->d_vinv, n * sizeof(float)));
    MDC_HIP(c, hipMemcpy(c->d_vinv, vignette_inv, n * sizeof(float), hipMemcpyHostToDevice));
  }
  return MDC_OK;
}

int mdc_set_remap(mdc_ctx* c, const float* rx, const float* ry, int in_w, int in_h, int out_w, int out_h) try {
  if (!c) return MDC_ERR_ARG;
  WriteLock lk(c->mu);
  return set_remap_locked(c, rx, ry, in_w, in_h, out_w, out_h);
} MDC_CATCH(c)

static int set_remap_locked(mdc_ctx* c, const float* rx, const float* ry, int in_w, int in_h, int out_w, int out_h) {
  DeviceGuard dg(c->device);
  MDC_HIP(c, hipDeviceSynchronize());
  c->valid_remap = false;
  c->tuned_fpb = 0;
  free_plan(c);
  for (float** p : {&c->d_rx, &c->d_ry})
    if (*p) {
      (void)hipFree(*p);
      *p = nullptr;
    }
  c->h_rx.clear();
  c->h_ry.clear();
  if (!rx || !ry) return MDC_OK;
  if (in_w <= 1 || in_h <= 1 || out_w <= 0 || out_h <= 0)
    return fail(c, MDC_ERR_ARG, "bad remap geometry %dx%d -> %dx%d", in_w, in_h, out_w, out_h);
  const size_t n = (size_t)out_w * out_h;
  // Defensive validation of what UndistorterFOV's constructor guarantees
  // (src/FOVUndistorter.cpp:243): every non-black tap lies strictly inside the frame.
  for (size_t i = 0; i < n; i++) {
    if (rx[i] < 0) continue;
    if (!(rx[i] > 0 && ry[i] > 0 && rx[i] < in_w - 1 && ry[i] < in_h - 1))
      return fail(c, MDC_ERR_ARG, "remap entry %zu = (%g,%g) is outside (0,%d)x(0,%d)", i, rx[i], ry[i], in_w - 1,
                  in_h - 1);
  }
  c->h_rx.assign(rx, rx + n);
  c->h_ry.assign(ry, ry + n);
  c->rm_in_w = in_w;
  c->rm_in_h = in_h;
  c->out_w = out_w;
  c->out_h = out_h;
  MDC_HIP(c, hipMalloc(&c->d_rx, n * sizeof(float)));
  MDC_HIP(c, hipMalloc(&c->d_ry, n * sizeof(float)));
  MDC_HIP(c, hipMemcpy(c->d_rx, rx, n * sizeof(float), hipMemcpyHostToDevice));
  MDC_HIP(c, hipMemcpy(c->d_ry, ry, n * sizeof(float), hipMemcpyHostToDevice));
  int rc = plan_tiles(c);
  if (rc != MDC_OK) return rc;
  c->valid_remap = true;
  return MDC_OK;
}

int mdc_synchronize(mdc_ctx* c) try {
  if (!c) return MDC_ERR_ARG;
  ReadLock lk(c->mu);
  DeviceGuard dg(c->device);
  std::vector<hipStream_t> streams;
  {
    std::lock_guard<std::mutex> sl(c->slot_mu);
    for (mdc_ctx::HostSlot* h : c->slots) streams.push_back(h->stream);
  }
  for (int k = 0; k < 2; k++)
    if (c->pipe_stream[k]) streams.push_back(c->pipe_stream[k]);
  if (c->pipe_up_stream) streams.push_back(c->pipe_up_stream);
  for (hipStream_t st : streams) MDC_HIP(c, hipStreamSynchronize(st));
  return MDC_OK;
} MDC_CATCH(c)

// ---- table hand-over ------------------------------------------------------------------

int mdc_export_tables(mdc_ctx* c, void* blob, size_t cap, size_t* size) try {
  if (!c || !size) return MDC_ERR_ARG;
  ReadLock lk(c->mu);
  const size_t nv = c->valid_vignette ? c->h_vinv.size() : 0;
  const size_t nr = c->valid_remap ? c->h_rx.size() : 0;
  const size_t need = sizeof(BlobHeader) + 256 * 4 + nv * 4 + 2 * nr * 4;
  *size = need;
  if (!blob) return MDC_OK;
  if (cap < need) return fail(c, MDC_ERR_ARG, "export buffer too small (%zu < %zu)", cap, need);
  BlobHeader h{kMagic, 1, c->in_w, c->in_h, c->rm_in_w, c->rm_in_h, c->out_w, c->out_h,
               c->valid_gamma, c->valid_vignette, c->valid_remap, 0};
  char* p = (char*)blob;
  memcpy(p, &h, sizeof h);
  p += sizeof h;
  if (c->valid_gamma) memcpy(p, c->h_ginv.data(), 256 * 4);
  else memset(p, 0, 256 * 4);
  p += 256 * 4;
  if (nv) memcpy(p, c->h_vinv.data(), nv * 4);
  p += nv * 4;
  if (nr) {
    memcpy(p, c->h_rx.data(), nr * 4);
    p += nr * 4;
    memcpy(p, c->h_ry.data(), nr * 4);
  }
  return MDC_OK;
} MDC_CATCH(c)

int mdc_import_tables(mdc_ctx* c, const void* blob, size_t size) try {
  if (!c || !blob) return MDC_ERR_ARG;
  BlobHeader h;
  if (size < sizeof h) return fail(c, MDC_ERR_ARG, "table blob truncated");
  memcpy(&h, blob, sizeof h);
  if (h.magic != kMagic || h.version != 1) return fail(c, MDC_ERR_ARG, "table blob has wrong magic/version");
  const size_t nv = h.valid_vignette ? (size_t)h.in_w * h.in_h : 0;
  const size_t nr = h.valid_remap ? (size_t)h.out_w * h.out_h : 0;
  if (size != sizeof h + 256 * 4 + nv * 4 + 2 * nr * 4) return fail(c, MDC_ERR_ARG, "table blob has wrong size");
  const char* p = (const char*)blob + sizeof h;
  const float* ginv = (const float*)p;
  p += 256 * 4;
  const float* vinv = (const float*)p;
  p += nv * 4;
  const float* rx = (const float*)p;
  const float* ry = rx + nr;
  // one critical section: no other thread may see the new photometric tables next to the old remap
  WriteLock lk(c->mu);
  int rc = MDC_OK;
  if (h.in_w > 0 && h.in_h > 0) {
    rc = set_photometric_locked(c, h.valid_gamma ? ginv : nullptr, h.valid_vignette ? vinv : nullptr, h.in_w, h.in_h);
  } else {  // the blob carries no photometric calibration: neither does the context afterwards
    DeviceGuard dg(c->device);
    MDC_HIP(c, hipDeviceSynchronize());
    c->in_w = c->in_h = 0;
    c->valid_gamma = c->valid_vignette = false;
    c->h_vinv.clear();
    if (c->d_vinv) {
      (void)hipFree(c->d_vinv);
      c->d_vinv = nullptr;
    }
    rc = upload_luts(c);
  }
  if (rc != MDC_OK) return rc;
  if (h.valid_remap) rc = set_remap_locked(c, rx, ry, h.rm_in_w, h.rm_in_h, h.out_w, h.out_h);
  else rc = set_remap_locked(c, nullptr, nullptr, 0, 0, 0, 0);
  return rc;
} MDC_CATCH(c)

}  // extern "C"

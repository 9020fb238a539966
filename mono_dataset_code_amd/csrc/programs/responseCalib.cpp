// responseCalib: drop-in for the reference's program of the same name (src/main_responseCalib.cpp:149-380).  Same arguments
// (folder, leakPadding=, iterations=, skip=) plus order=exact|direct and plots=0|1, same console lines, same photoCalibResult/log.txt
// and photoCalibResult/pcalib.txt, and with plots=1 (the default) the reference's result images: E-0.png, E-016.png and per iteration
// G-k.png, E-k.png, E-k16.png, rendered by mdc_rcal_plot_e_device / mdc_rcal_plot_g_device and encoded by libmdc_pngw.so (gray) and
// libmdc_pngw_rgb.so (colour), with the "Irradiance" / "Inv. Response" lines where the reference prints them (:272-273, :307-310, :342-345).  With plots=1 the iteration
// runs through the step calls (the same kernels in the same order as mdc_rcal_solve_device: pcalib.txt and log.txt do not depend
// on the switch).  Only the host side lives here: the frames go from the reader's decode pool straight into a device
// stack (DatasetReader::getImagesRawDevice) and every computation on the stack is a call of include/mdc_hip.h (mdc_rcal_*).
// Deviations: no plot windows (cv::imshow); photoCalibResult/ is created if missing and its files are overwritten -- nothing is
// deleted (the reference runs "rm -rf photoCalibResult").  With plots=0 the folder is created after the solve, as before the pictures
// existed; with plots=1 before the first picture, as the reference does: a failure in the loop then leaves the folder and what was written.
#include <sys/stat.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "BenchmarkDatasetReader.h"
#include "mdc_hip.h"
#include "mdc_pngw.h"
#include "mdc_pngw_rgb.h"

static int leakPadding = 2;
static int nits = 10;
static int skipFrames = 1;
static unsigned order = MDC_RCAL_EXACT_ORDER;
static int plots = 1;

static void parseArgument(char* arg) {  // :149-173
  int option;
  char word[32];
  if (1 == sscanf(arg, "leakPadding=%d", &option)) {
    leakPadding = option;
    printf("leakPadding set to %d!\n", leakPadding);
    return;
  }
  if (1 == sscanf(arg, "iterations=%d", &option)) {
    nits = option;
    printf("nits set to %d!\n", nits);
    return;
  }
  if (1 == sscanf(arg, "skip=%d", &option)) {
    skipFrames = option;
    printf("skipFrames set to %d!\n", skipFrames);
    return;
  }
  if (1 == sscanf(arg, "plots=%d", &option) && (option == 0 || option == 1)) {
    plots = option;
    printf("plots set to %d!\n", plots);
    return;
  }
  if (1 == sscanf(arg, "order=%31s", word) && (!strcmp(word, "exact") || !strcmp(word, "direct"))) {
    order = strcmp(word, "exact") ? MDC_RCAL_DIRECT : MDC_RCAL_EXACT_ORDER;
    printf("order set to %s!\n", word);
    return;
  }
  printf("could not parse argument \"%s\"!!\n", arg);
}

static int die(mdc_ctx* ctx, const char* what) {
  fprintf(stderr, "responseCalib: %s: %s\n", what, mdc_last_error(ctx));
  return 1;
}

// One PNG encoder (gray: mdc_pngw.h, colour: mdc_pngw_rgb.h) with its own output slot; write() brings the file to the host and saves it.
struct PngOut {
  mdc_ctx* ctx;
  bool colour;
  mdcp_encoder* enc;
  uint8_t* d_png;
  int64_t slot;
  int32_t* d_size;
  explicit PngOut(bool colour_) : ctx(0), colour(colour_), enc(0), d_png(0), slot(0), d_size(0) {}
  ~PngOut() {
    if (colour) mdcp_destroy_rgb8(enc);
    else mdcp_destroy(enc);
  }
  const char* error() const { return colour ? mdcp_last_error_rgb8() : mdcp_last_error(); }
  bool ready(mdc_ctx* c, int rc) {
    ctx = c;
    if (rc == MDCP_OK) rc = colour ? mdcp_output_device_rgb8(enc, &d_png, &slot, &d_size) : mdcp_output_device(enc, &d_png, &slot, &d_size);
    if (rc != MDCP_OK) fprintf(stderr, "responseCalib: %s\n", error());
    return rc == MDCP_OK;
  }
  bool write(int rc, const char* path) {
    if (rc != MDCP_OK) {
      fprintf(stderr, "responseCalib: %s: %s\n", path, error());
      return false;
    }
    int32_t size = 0;
    std::vector<uint8_t> file;
    if (mdc_copy_to_host(ctx, &size, d_size, sizeof size) != MDC_OK || size <= 0 || size > slot ||
        (file.resize((size_t)size), mdc_copy_to_host(ctx, file.data(), d_png, (size_t)size)) != MDC_OK) {
      fprintf(stderr, "responseCalib: reading %s back failed: %s\n", path, mdc_last_error(ctx));
      return false;
    }
    FILE* f = fopen(path, "wb");
    bool ok = f && fwrite(file.data(), 1, file.size(), f) == file.size();
    if (f && fclose(f) != 0) ok = false;
    if (!ok) fprintf(stderr, "responseCalib: could not write %s\n", path);
    return ok;
  }
};

// plotE / plotG (:72-146) without the windows: the render calls, the encoders and the device arrays between them
struct Plots {
  mdc_ctx* ctx;
  int w, h;
  PngOut rgb, e16, g8;
  uint8_t* d_rgb;
  uint16_t* d_e16;
  float* d_gimg;
  Plots() : ctx(0), w(0), h(0), rgb(true), e16(false), g8(false), d_rgb(0), d_e16(0), d_gimg(0) {}
  bool init(mdc_ctx* c, int device, int w_, int h_) {
    ctx = c, w = w_, h = h_;
    const size_t frame = (size_t)w * h;
    if (!rgb.ready(c, mdcp_create_rgb8(device, w, h, MDCP_FILTER_ADAPTIVE, 1, &rgb.enc)) ||
        !e16.ready(c, mdcp_create(device, w, h, 16, MDCP_FILTER_ADAPTIVE, 1, &e16.enc)) ||
        !g8.ready(c, mdcp_create(device, 256, 256, 8, MDCP_FILTER_ADAPTIVE, 1, &g8.enc)))
      return false;
    if (mdc_device_alloc(c, frame * 3, (void**)&d_rgb) != MDC_OK || mdc_device_alloc(c, frame * sizeof(uint16_t), (void**)&d_e16) != MDC_OK ||
        mdc_device_alloc(c, 256 * 256 * sizeof(float), (void**)&d_gimg) != MDC_OK) {
      fprintf(stderr, "responseCalib: plot buffers: %s\n", mdc_last_error(c));
      return false;
    }
    return true;
  }
  ~Plots() {
    if (d_rgb) mdc_device_free(ctx, d_rgb);
    if (d_e16) mdc_device_free(ctx, d_e16);
    if (d_gimg) mdc_device_free(ctx, d_gimg);
  }
  // saveTo + ".png" and saveTo + "16.png"; range = Emin, Emax of the "Irradiance" line, which the caller prints at the reference's place
  bool plotE(const double* d_E, const std::string& saveTo, double* range) {
    if (mdc_rcal_plot_e_device(ctx, d_E, w, h, d_rgb, d_e16, range, 0) != MDC_OK) {
      fprintf(stderr, "responseCalib: plotE: %s\n", mdc_last_error(ctx));
      return false;
    }
    const int64_t frame = (int64_t)w * h;
    return rgb.write(mdcp_encode_rgb8_device(rgb.enc, d_rgb, frame * 3, 1, rgb.d_png, rgb.slot, rgb.d_size, 0), (saveTo + ".png").c_str()) &&
           e16.write(mdcp_encode_u16_device(e16.enc, d_e16, frame, 1, e16.d_png, e16.slot, e16.d_size, 0), (saveTo + "16.png").c_str());
  }
  bool plotG(const double* d_G, const std::string& saveTo) {
    double range[2];
    if (mdc_rcal_plot_g_device(ctx, d_G, d_gimg, range, 0) != MDC_OK) {
      fprintf(stderr, "responseCalib: plotG: %s\n", mdc_last_error(ctx));
      return false;
    }
    printf("Inv. Response %f - %f\n", range[0], range[1]);
    return g8.write(mdcp_encode_f32_device(g8.enc, d_gimg, 256 * 256, 1, g8.d_png, g8.slot, g8.d_size, 0), saveTo.c_str());
  }
};

// The loop of mdc_rcal_solve_device (:250-358) through the step calls, with the pictures and their lines at the reference's places.
// *index and *d_pairs are the caller's to release, whatever the outcome.
static int solveWithPlots(mdc_ctx* ctx, Plots& plot, int dev, const uint8_t* d_stack, const double* d_exposure, int n, int w, int h, double* d_G,
                          double* d_E, std::ofstream& logFile, mdc_rcal_index** index_out, double** d_pairs_out) {
  if (!plot.init(ctx, dev, w, h)) return 1;
  std::vector<double> G(256);
  double pairs[8], range[2];  // pairs = {rmse, num} x 4: init, after the G step, after the E step, after the rescale
  const std::vector<double> zeros(256, 0.0);
  if (mdc_device_alloc(ctx, sizeof pairs, (void**)d_pairs_out) != MDC_OK) return die(ctx, "device buffers");
  double* d_pairs = *d_pairs_out;
  if (order == MDC_RCAL_EXACT_ORDER && nits > 0 && mdc_rcal_index_create(ctx, d_stack, n, w, h, 0, index_out) != MDC_OK) return die(ctx, "index");
  mdc_rcal_index* index = *index_out;
  if (mdc_copy_to_device(ctx, d_G, zeros.data(), 256 * sizeof(double)) != MDC_OK || mdc_rcal_init_e_device(ctx, d_stack, n, w, h, d_E, 0) != MDC_OK ||
      mdc_rcal_rmse_device(ctx, d_stack, d_exposure, n, w, h, d_G, d_E, d_pairs, 0) != MDC_OK ||
      mdc_copy_to_host(ctx, pairs, d_pairs, 2 * sizeof(double)) != MDC_OK)
    return die(ctx, "initial irradiance");
  printf("init RMSE = %f! \t", pairs[0]);
  if (!plot.plotE(d_E, "photoCalibResult/E-0", range)) return 1;
  printf("Irradiance %f - %f\n", range[0], range[1]);
  for (int it = 0; it < nits; it++) {
    char buf[1000];
    if ((index ? mdc_rcal_g_step_indexed_device(ctx, index, d_exposure, d_E, d_G, 0) : mdc_rcal_g_step_device(ctx, d_stack, d_exposure, n, w, h, d_E, d_G, 0)) != MDC_OK)
      return die(ctx, "G step");
    if (mdc_rcal_e_step_device(ctx, d_stack, d_exposure, n, w, h, d_G, d_E, d_pairs + 2, 0) != MDC_OK) return die(ctx, "E step");
    if (mdc_copy_to_host(ctx, pairs + 2, d_pairs + 2, 2 * sizeof(double)) != MDC_OK || mdc_copy_to_host(ctx, G.data(), d_G, 256 * sizeof(double)) != MDC_OK)
      return die(ctx, "download");
    printf("optG RMSE = %f! \t", pairs[2]);
    snprintf(buf, sizeof buf, "photoCalibResult/G-%d.png", it + 1);
    if (!plot.plotG(d_G, buf)) return 1;
    // the E picture is of E before the rescale, whose call also measures "OptE RMSE": rendered now, its line printed after that one
    snprintf(buf, sizeof buf, "photoCalibResult/E-%d", it + 1);
    if (!plot.plotE(d_E, buf, range)) return 1;
    const double rescaleFactor = 255.0 / G[255];  // :350
    if (mdc_rcal_rescale_device(ctx, d_stack, d_exposure, n, w, h, d_G, d_E, d_pairs + 4, d_pairs + 6, 0) != MDC_OK) return die(ctx, "rescale");
    if (mdc_copy_to_host(ctx, pairs + 4, d_pairs + 4, 4 * sizeof(double)) != MDC_OK) return die(ctx, "download");
    printf("OptE RMSE = %f!  \t", pairs[4]);
    printf("Irradiance %f - %f\n", range[0], range[1]);
    printf("resc RMSE = %f!  \trescale with %f!\n", pairs[6], rescaleFactor);
    logFile << it << " " << n << " " << pairs[7] << " " << pairs[6] << "\n";
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <dataset folder> [leakPadding=2] [iterations=10] [skip=1] [order=exact|direct] [plots=1]\n", argv[0]);
    return 1;
  }
  for (int i = 2; i < argc; i++) parseArgument(argv[i]);
  if (skipFrames < 1) {
    fprintf(stderr, "responseCalib: skip must be at least 1\n");
    return 1;
  }
  if (nits < 0) nits = 0;

  std::string folder = argv[1];
  if (folder.empty() || folder[folder.size() - 1] != '/') folder += "/";
  DatasetReader* reader = new DatasetReader(folder);
  int w = 0, h = 0;
  reader->getRawSize(&w, &h);
  const int total = reader->getNumImages();
  const int count = total > 0 ? (total - 1) / skipFrames + 1 : 0;  // ids 0, skip, 2*skip, ... (:191)
  if (w <= 0 || h <= 0 || count <= 0) {
    printf("loaded %d images\n", 0);
    fprintf(stderr, "responseCalib: no decodable frame in %s\n", folder.c_str());
    delete reader;
    return 1;
  }
  const size_t frame = (size_t)w * h;

  mdc_ctx* ctx = 0;
  const int dev = reader->getDevice() >= 0 ? reader->getDevice() : 0;
  if (mdc_create(dev, &ctx) != MDC_OK) return die(0, "no GPU");
  uint8_t* d_stack = 0;
  if (mdc_device_alloc(ctx, (size_t)count * frame, (void**)&d_stack) != MDC_OK) return die(ctx, "device stack");
  std::vector<unsigned char> valid((size_t)count, 0);
  reader->getImagesRawDevice(0, count, skipFrames, d_stack, valid.data());

  // :193-206: empty frames are skipped, a size different from the first frame's ends the program
  std::vector<double> exposure;
  int n = 0;
  for (int j = 0; j < count; j++) {
    const int id = j * skipFrames;
    if (!valid[(size_t)j]) {
      int fw = 0, fh = 0;
      (void)reader->getImageRaw(id, &fw, &fh);  // header size of a frame that did not come through (0 x 0: undecodable)
      if (fw > 0 && fh > 0 && fw != w) {
        printf("width mismatch!\n");
        exit(1);
      }
      if (fw > 0 && fh > 0 && fh != h) {
        printf("height mismatch!\n");
        exit(1);
      }
      continue;
    }
    if (n != j && mdc_copy_to_device(ctx, d_stack + (size_t)n * frame, d_stack + (size_t)j * frame, frame) != MDC_OK)
      return die(ctx, "compacting the stack");
    exposure.push_back((double)reader->getExposure(id));
    n++;
  }
  printf("loaded %d images\n", n);
  if (n == 0) {
    fprintf(stderr, "responseCalib: no frame could be loaded\n");
    return 1;
  }

  double *d_exposure = 0, *d_G = 0, *d_E = 0;
  if (mdc_device_alloc(ctx, (size_t)n * sizeof(double), (void**)&d_exposure) != MDC_OK ||
      mdc_device_alloc(ctx, 256 * sizeof(double), (void**)&d_G) != MDC_OK || mdc_device_alloc(ctx, frame * sizeof(double), (void**)&d_E) != MDC_OK)
    return die(ctx, "device buffers");
  if (mdc_copy_to_device(ctx, d_exposure, exposure.data(), (size_t)n * sizeof(double)) != MDC_OK) return die(ctx, "exposure upload");
  if (mdc_rcal_leak_pad_device(ctx, d_stack, n, w, h, leakPadding, 0) != MDC_OK) return die(ctx, "leak padding");

  std::vector<double> G(256);
  std::vector<mdc_rcal_iter> iters((size_t)(nits > 0 ? nits : 1));
  mdc_rcal_log log;
  log.iters = iters.data();
  if (!plots && mdc_rcal_solve_device(ctx, d_stack, d_exposure, n, w, h, nits, order, d_G, d_E, &log, 0) != MDC_OK) return die(ctx, "solve");

  if (mkdir("photoCalibResult", 0755) != 0 && errno != EEXIST) {
    fprintf(stderr, "responseCalib: could not create photoCalibResult folder!\n");
    return 1;
  }
  std::ofstream logFile;
  logFile.open("photoCalibResult/log.txt", std::ios::trunc | std::ios::out);
  logFile.precision(15);
  if (!plots) {
    printf("init RMSE = %f! \t", log.init_rmse);
    for (int it = 0; it < nits; it++) {
      const mdc_rcal_iter& r = iters[(size_t)it];
      printf("optG RMSE = %f! \t", r.rmse_G);
      printf("OptE RMSE = %f!  \t", r.rmse_E);
      printf("resc RMSE = %f!  \trescale with %f!\n", r.rmse_resc, r.rescale);
      logFile << it << " " << n << " " << r.num_resc << " " << r.rmse_resc << "\n";
    }
  } else {
    Plots plot;
    mdc_rcal_index* index = 0;
    double* d_pairs = 0;
    const int rc = solveWithPlots(ctx, plot, dev, d_stack, d_exposure, n, w, h, d_G, d_E, logFile, &index, &d_pairs);
    mdc_rcal_index_destroy(index);
    if (d_pairs) mdc_device_free(ctx, d_pairs);
    if (rc) return rc;
  }
  logFile.flush();
  logFile.close();
  if (mdc_copy_to_host(ctx, G.data(), d_G, 256 * sizeof(double)) != MDC_OK) return die(ctx, "result download");

  std::ofstream lg;
  lg.open("photoCalibResult/pcalib.txt", std::ios::trunc | std::ios::out);
  lg.precision(15);
  for (int i = 0; i < 256; i++) lg << G[(size_t)i] << " ";
  lg << "\n";
  lg.flush();
  lg.close();
  if (!lg) {
    fprintf(stderr, "responseCalib: could not write photoCalibResult/pcalib.txt\n");
    return 1;
  }

  mdc_device_free(ctx, d_E);
  mdc_device_free(ctx, d_G);
  mdc_device_free(ctx, d_exposure);
  mdc_device_free(ctx, d_stack);
  mdc_destroy(ctx);
  delete reader;
  return 0;
}

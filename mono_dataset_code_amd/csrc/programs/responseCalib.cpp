// responseCalib: drop-in for the reference's program of the same name (src/main_responseCalib.cpp:149-380).  Same arguments
// (folder, leakPadding=, iterations=, skip=) plus order=exact|direct, same console RMSE lines, same photoCalibResult/log.txt and
// photoCalibResult/pcalib.txt.  Only the host side lives here: the frames go from the reader's decode pool straight into a device
// stack (DatasetReader::getImagesRawDevice) and every computation on the stack is a call of include/mdc_hip.h (mdc_rcal_*).
// Deviations: no plot windows or PNG dumps (plotE / plotG, with their "Irradiance" / "Inv. Response" lines); photoCalibResult/
// is created if missing and the two files are overwritten -- nothing is deleted (the reference runs "rm -rf photoCalibResult").
#include <sys/stat.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "BenchmarkDatasetReader.h"
#include "mdc_hip.h"

static int leakPadding = 2;
static int nits = 10;
static int skipFrames = 1;
static unsigned order = MDC_RCAL_EXACT_ORDER;

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

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <dataset folder> [leakPadding=2] [iterations=10] [skip=1] [order=exact|direct]\n", argv[0]);
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

  std::vector<mdc_rcal_iter> iters((size_t)(nits > 0 ? nits : 1));
  mdc_rcal_log log;
  log.iters = iters.data();
  if (mdc_rcal_solve_device(ctx, d_stack, d_exposure, n, w, h, nits, order, d_G, d_E, &log, 0) != MDC_OK) return die(ctx, "solve");
  std::vector<double> G(256);
  if (mdc_copy_to_host(ctx, G.data(), d_G, 256 * sizeof(double)) != MDC_OK) return die(ctx, "result download");

  if (mkdir("photoCalibResult", 0755) != 0 && errno != EEXIST) {
    fprintf(stderr, "responseCalib: could not create photoCalibResult folder!\n");
    return 1;
  }
  std::ofstream logFile;
  logFile.open("photoCalibResult/log.txt", std::ios::trunc | std::ios::out);
  logFile.precision(15);
  printf("init RMSE = %f! \t", log.init_rmse);
  for (int it = 0; it < nits; it++) {
    const mdc_rcal_iter& r = iters[(size_t)it];
    printf("optG RMSE = %f! \t", r.rmse_G);
    printf("OptE RMSE = %f!  \t", r.rmse_E);
    printf("resc RMSE = %f!  \trescale with %f!\n", r.rmse_resc, r.rescale);
    logFile << it << " " << n << " " << r.num_resc << " " << r.rmse_resc << "\n";
  }
  logFile.flush();
  logFile.close();

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

// playDataset: the reference's program of the same name (src/main_playbackDataset.cpp) in its saving mode.  Same header lines
// on stdout (:55-70); with a second argument, "Saving undistorted Dataset to here!" and %05d.jpg of every frame in the current
// directory (:73-85) -- the frames of getImage(i, true, false, false, false), the bytes cv::imwrite gives a CV_32F image at its
// default quality 95.  Only the host side lives here: chunks of frames go through DatasetReader::getImagesDevice into a device
// array, include/mdc_jenc.h encodes them there, and only the encoded bytes and their sizes come back.
// Deviations: the interactive viewer (:92-128) is not built -- with one argument the program prints the header and says so; a
// frame the reader cannot deliver is skipped with a message (the reference dereferences the null image).
#include <cstdio>
#include <cstdlib>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "BenchmarkDatasetReader.h"
#include "mdc_hip.h"
#include "mdc_jenc.h"

// operator<< of Eigen's default IOFormat on a 3 x 3 float matrix: stream precision, columns right-aligned to the widest
// coefficient, one blank between them (the Eigen stand-in of this tree has no stream operator; real Eigen prints the same)
static void print3x3(const Eigen::Matrix3f& K) {
  std::string cell[9];
  size_t width = 0;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      std::ostringstream s;
      s << K(r, c);
      cell[r * 3 + c] = s.str();
      if (cell[r * 3 + c].size() > width) width = cell[r * 3 + c].size();
    }
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) std::cout << (c ? " " : "") << std::setw((int)width) << cell[r * 3 + c];
    if (r < 2) std::cout << "\n";
  }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <dataset folder> [anything: save every rectified frame as %%05d.jpg into the current directory]\n", argv[0]);
    return 1;
  }
  std::string dataset = argv[1];
  printf("Playback dataset %s!\n", dataset.c_str());
  if (dataset.empty() || dataset[dataset.size() - 1] != '/') dataset += "/";  // the reader wants the trailing slash
  DatasetReader* reader = new DatasetReader(dataset);

  Eigen::Matrix3f K_rect = reader->getUndistorter()->getK_rect();
  Eigen::Vector2i dim_rect = reader->getUndistorter()->getOutputDims();
  printf("Rectified Images: %d x %d. K:\n", dim_rect[0], dim_rect[1]);
  fflush(stdout);
  print3x3(K_rect);
  std::cout << "\n\n" << std::flush;

  Eigen::Matrix3f K_org = reader->getUndistorter()->getK_org();
  Eigen::Vector2i dim_org = reader->getUndistorter()->getInputDims();
  float omega = reader->getUndistorter()->getOmega();
  printf("Original Images: %d x %d. omega=%f K:\n", dim_org[0], dim_org[1], omega);
  fflush(stdout);
  print3x3(K_org);
  std::cout << "\n\n" << std::flush;

  if (argc <= 2) {
    printf("The interactive viewer is not built: give a second argument to save the undistorted dataset as JPEG.\n");
    delete reader;
    return 0;
  }

  printf("Saving undistorted Dataset to here!\n");
  const int w = dim_rect[0], h = dim_rect[1], total = reader->getNumImages();
  mdc_ctx* ctx = reader->getContext();
  if (!ctx || w <= 0 || h <= 0) {
    fprintf(stderr, "playDataset: no GPU context (or no valid calibration) behind the reader: nothing saved\n");
    delete reader;
    return 1;
  }
  const int chunk = total < 128 ? (total > 0 ? total : 1) : 128;
  const size_t frame = (size_t)w * h;
  mdcj_encoder* enc = 0;
  if (mdcj_create(reader->getDevice(), w, h, 95, chunk, &enc) != MDCJ_OK) {
    fprintf(stderr, "playDataset: %s\n", mdcj_last_error());
    return 1;
  }
  float* d_frames = 0;
  uint8_t* d_out = 0;
  int32_t* d_sizes = 0;
  int64_t slot = 0;
  if (mdc_device_alloc(ctx, (size_t)chunk * frame * sizeof(float), (void**)&d_frames) != MDC_OK) {
    fprintf(stderr, "playDataset: %s\n", mdc_last_error(ctx));
    return 1;
  }
  if (mdcj_output_device(enc, &d_out, &slot, &d_sizes) != MDCJ_OK) {
    fprintf(stderr, "playDataset: %s\n", mdcj_last_error());
    return 1;
  }
  std::vector<unsigned char> valid((size_t)chunk);
  std::vector<int32_t> sizes((size_t)chunk);
  std::vector<uint8_t> bytes((size_t)chunk * (size_t)slot);
  int status = 0;
  for (int first = 0; first < total && !status; first += chunk) {
    const int n = total - first < chunk ? total - first : chunk;
    mdc_device_outputs outs = mdc_device_outputs();
    outs.base = d_frames;
    outs.levels = 1;
    reader->getImagesDevice(first, n, true, false, false, false, &outs, valid.data());
    if (mdc_synchronize(ctx) != MDC_OK) {
      fprintf(stderr, "playDataset: %s\n", mdc_last_error(ctx));
      status = 1;
      break;
    }
    // positions without a frame are encoded too (whatever they hold is a legal input) and not written
    if (mdcj_encode_f32_device(enc, d_frames, (int64_t)frame, n, d_out, slot, d_sizes, 0) != MDCJ_OK ||
        mdcj_fetch(enc, d_out, slot, d_sizes, n, bytes.data(), (int64_t)bytes.size(), sizes.data(), 0) < 0) {
      fprintf(stderr, "playDataset: %s\n", mdcj_last_error());
      status = 1;
      break;
    }
    size_t at = 0;
    for (int i = 0; i < n; i++) {
      if (!valid[(size_t)i]) {
        printf("frame %d could not be read: skipped\n", first + i);
      } else {
        char buf[1000];
        snprintf(buf, 1000, "%05d.jpg", first + i);
        FILE* f = fopen(buf, "wb");
        if (!f || fwrite(bytes.data() + at, 1, (size_t)sizes[(size_t)i], f) != (size_t)sizes[(size_t)i]) {
          fprintf(stderr, "playDataset: cannot write %s\n", buf);
          status = 1;
        }
        if (f) fclose(f);
      }
      at += (size_t)sizes[(size_t)i];
    }
  }
  mdc_device_free(ctx, d_frames);
  mdcj_destroy(enc);
  delete reader;
  return status;
}

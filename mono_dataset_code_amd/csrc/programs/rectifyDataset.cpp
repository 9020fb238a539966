// rectifyDataset <dataset folder> <output folder> [quality=95]: a sequence, rectified, as a dataset of its own.
// The frames are those of playDataset's saving mode -- getImage(i, true, false, false, false), encoded by include/mdc_jenc.h with the
// bytes cv::imwrite gives a CV_32F image -- but they go into one images.zip of stored %05d.jpg entries, built on the device by
// include/mdc_zipw.h, and the folder gets what a reader needs to open it:
//   images.zip   entry %05d.jpg of frame i: exactly the file `playDataset <folder> x` writes for it
//   camera.txt   the rectified pinhole: "fx/w fy/h (cx+0.5)/w (cy+0.5)/h 0" of getK_rect() / getOutputDims() (each %.9g), "w h", "crop",
//                "w h" -- with omega = 0 a reader takes the relative intrinsics as they are (the reference's src/FOVUndistorter.cpp:144-150)
//   times.txt    the source's lines, verbatim, of the frames that were written (only if the source has the file)
//   pcalib.txt   copied verbatim (if present)
// vignette.png is NOT exported: a rectified vignette needs a 16-bit PNG writer and a decision about the black border pixels, so the
// exported dataset opens with validVignette == false, as any dataset without that file does.
// The output folder is created if missing; files of these names are overwritten, nothing is deleted.  A frame the reader cannot
// deliver is reported and left out (of images.zip and of times.txt).
#include <sys/stat.h>
#include <sys/types.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "BenchmarkDatasetReader.h"
#include "mdc_hip.h"
#include "mdc_jenc.h"
#include "mdc_zipw.h"

static bool make_dirs(const std::string& path) {
  for (size_t at = 1; at <= path.size(); at++) {
    if (at != path.size() && path[at] != '/') continue;
    const std::string part = path.substr(0, at);
    if (mkdir(part.c_str(), 0777) != 0 && errno != EEXIST) return false;
  }
  struct stat st;
  return stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

static bool copy_file(const std::string& from, const std::string& to) {
  std::ifstream in(from.c_str(), std::ios::binary);
  if (!in.good()) return false;
  std::ofstream out(to.c_str(), std::ios::binary | std::ios::trunc);
  out << in.rdbuf();
  return out.good();
}

// the lines of times.txt the reader takes a frame's time from, in frame order (DatasetReader: "id stamp exposure" or "id stamp")
static std::vector<std::string> time_lines(const std::string& file, bool* present) {
  std::vector<std::string> lines;
  std::ifstream tr(file.c_str());
  *present = tr.good();
  std::string line;
  while (tr.good() && std::getline(tr, line)) {
    int id;
    double stamp;
    if (2 == std::sscanf(line.c_str(), "%d %lf", &id, &stamp)) lines.push_back(line);
  }
  return lines;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s <dataset folder> <output folder> [quality=95]\n", argv[0]);
    return 1;
  }
  std::string dataset = argv[1], out = argv[2];
  const int quality = argc > 3 ? atoi(argv[3]) : 95;
  if (dataset.empty() || dataset[dataset.size() - 1] != '/') dataset += "/";  // the reader wants the trailing slash
  while (out.size() > 1 && out[out.size() - 1] == '/') out.erase(out.size() - 1);
  if (out.empty() || !make_dirs(out)) {
    fprintf(stderr, "rectifyDataset: cannot create %s: %s\n", out.c_str(), strerror(errno));
    return 1;
  }
  DatasetReader* reader = new DatasetReader(dataset);
  Eigen::Matrix3f K = reader->getUndistorter()->getK_rect();
  Eigen::Vector2i dim = reader->getUndistorter()->getOutputDims();
  const int w = dim[0], h = dim[1], total = reader->getNumImages();
  mdc_ctx* ctx = reader->getContext();
  if (!ctx || w <= 0 || h <= 0) {
    fprintf(stderr, "rectifyDataset: no GPU context (or no valid calibration) behind the reader: nothing written\n");
    delete reader;
    return 1;
  }
  printf("Rectifying %s: %d frames of %d x %d into %s (JPEG quality %d)\n", dataset.c_str(), total, w, h, out.c_str(), quality);

  const int chunk = total < 128 ? (total > 0 ? total : 1) : 128;
  const size_t frame = (size_t)w * h;
  mdcj_encoder* enc = 0;
  if (mdcj_create(reader->getDevice(), w, h, quality, chunk, &enc) != MDCJ_OK) {
    fprintf(stderr, "rectifyDataset: %s\n", mdcj_last_error());
    return 1;
  }
  float* d_frames = 0;
  uint8_t* d_out = 0;
  int32_t* d_sizes = 0;
  int64_t slot = 0;
  if (mdc_device_alloc(ctx, (size_t)chunk * frame * sizeof(float), (void**)&d_frames) != MDC_OK) {
    fprintf(stderr, "rectifyDataset: %s\n", mdc_last_error(ctx));
    return 1;
  }
  if (mdcj_output_device(enc, &d_out, &slot, &d_sizes) != MDCJ_OK) {
    fprintf(stderr, "rectifyDataset: %s\n", mdcj_last_error());
    return 1;
  }
  mdcz_writer* zip = 0;
  if (mdcz_open((out + "/images.zip").c_str(), reader->getDevice(), 0, &zip) != MDCZ_OK) {
    fprintf(stderr, "rectifyDataset: %s\n", mdcz_last_error());
    return 1;
  }
  std::vector<unsigned char> valid((size_t)chunk), written((size_t)(total > 0 ? total : 1), 0);
  int status = 0;
  long long frames_written = 0;
  for (int first = 0; first < total && !status; first += chunk) {
    const int n = total - first < chunk ? total - first : chunk;
    mdc_device_outputs outs = mdc_device_outputs();
    outs.base = d_frames;
    outs.levels = 1;
    reader->getImagesDevice(first, n, true, false, false, false, &outs, valid.data());
    if (mdc_synchronize(ctx) != MDC_OK) {
      fprintf(stderr, "rectifyDataset: %s\n", mdc_last_error(ctx));
      status = 1;
      break;
    }
    // positions without a frame are encoded too (whatever they hold is a legal input) and left out of the archive
    if (mdcj_encode_f32_device(enc, d_frames, (int64_t)frame, n, d_out, slot, d_sizes, 0) != MDCJ_OK) {
      fprintf(stderr, "rectifyDataset: %s\n", mdcj_last_error());
      status = 1;
      break;
    }
    if (mdcz_append_device(zip, d_out, slot, d_sizes, valid.data(), n, first, ".jpg", 0) != MDCZ_OK) {
      fprintf(stderr, "rectifyDataset: %s\n", mdcz_last_error());
      status = 1;
      break;
    }
    for (int i = 0; i < n; i++) {
      if (!valid[(size_t)i]) printf("frame %d could not be read: left out\n", first + i);
      else written[(size_t)(first + i)] = 1, frames_written++;
    }
  }
  mdc_device_free(ctx, d_frames);
  mdcj_destroy(enc);
  if (status) {
    mdcz_abort(zip);
    delete reader;
    return status;
  }
  const int64_t zip_bytes = mdcz_close(zip);
  if (zip_bytes < 0) {
    fprintf(stderr, "rectifyDataset: %s\n", mdcz_last_error());
    delete reader;
    return 1;
  }
  printf("images.zip: %lld frames, %lld bytes\n", frames_written, (long long)zip_bytes);

  {
    FILE* f = fopen((out + "/camera.txt").c_str(), "w");
    const float fw = (float)w, fh = (float)h;
    if (!f || fprintf(f, "%.9g %.9g %.9g %.9g 0\n%d %d\ncrop\n%d %d\n", K(0, 0) / fw, K(1, 1) / fh, (K(0, 2) + 0.5f) / fw, (K(1, 2) + 0.5f) / fh, w, h, w, h) < 0) {
      fprintf(stderr, "rectifyDataset: cannot write %s/camera.txt\n", out.c_str());
      status = 1;
    }
    if (f && fclose(f) != 0) status = 1;
  }
  bool has_times = false;
  const std::vector<std::string> lines = time_lines(dataset + "times.txt", &has_times);
  if (has_times && lines.size() != (size_t)total) {
    printf("times.txt has %zu lines for %d frames (the reader sets every time to zero): not exported\n", lines.size(), total);
  } else if (has_times) {
    std::ofstream tw((out + "/times.txt").c_str(), std::ios::binary | std::ios::trunc);
    for (int i = 0; i < total; i++)
      if (written[(size_t)i]) tw << lines[(size_t)i] << "\n";
    tw.close();
    if (!tw.good()) {
      fprintf(stderr, "rectifyDataset: cannot write %s/times.txt\n", out.c_str());
      status = 1;
    }
  }
  {
    std::ifstream probe((dataset + "pcalib.txt").c_str());
    if (probe.good() && !copy_file(dataset + "pcalib.txt", out + "/pcalib.txt")) {
      fprintf(stderr, "rectifyDataset: cannot write %s/pcalib.txt\n", out.c_str());
      status = 1;
    }
  }
  printf("vignette.png is not exported (a rectified vignette is out of scope): the dataset opens without a vignette.\n");
  delete reader;
  return status;
}

// rectifyDataset <dataset folder> <output folder> [quality=95] [frames=jpg|png] [vignette=0|1] [compress=huffman|lz77] [chain=N]
// [huffman=standard|optimal]: a sequence, rectified, as a dataset
// of its own.  The key=value arguments may stand in any position behind the two folders; a bare number is the JPEG quality.
// The frames are those of playDataset's saving mode -- getImage(i, true, false, false, false), encoded by include/mdc_jenc.h with the
// bytes cv::imwrite gives a CV_32F image -- but they go into one images.zip of stored %05d.jpg entries, built on the device by
// include/mdc_zipw.h, and the folder gets what a reader needs to open it:
//   images.zip   entry %05d.jpg of frame i: exactly the file `playDataset <folder> x` writes for it
//   camera.txt   the rectified pinhole: "fx/w fy/h (cx+0.5)/w (cy+0.5)/h 0" of getK_rect() / getOutputDims() (each %.9g), "w h", "crop",
//                "w h" -- with omega = 0 a reader takes the relative intrinsics as they are (the reference's src/FOVUndistorter.cpp:144-150)
//   times.txt    the source's lines, verbatim, of the frames that were written (only if the source has the file)
//   pcalib.txt   copied verbatim (if present)
// frames=png: images.zip holds %05d.png entries instead, 8-bit, lossless: the same rectified float frames converted as the JPEG
// encoder converts them (rintf, clamped to 0..255, NaN -> 0) and encoded on the device by include/mdc_pngw.h; no JPEG encoder is made.
// compress=lz77 (with frames=png only; chain=N, 1..64, default 4, is its match depth) encodes the frames, and vignette.png, by
// include/mdc_pnglz.h instead: the same pixels in files that are never larger.  Such files carry distance codes, which the reader
// decodes on the host unless MDC_GPU_PNG=2 sends them to the device decoder's general path or MDC_GPU_PNG=3 to the parallel inflate of
// include/mdc_pngdx.h.  The default, compress=huffman, writes
// today's files byte for byte.  A bad value is refused with one line before anything is opened or created.
// huffman=optimal (with frames=jpg only) encodes the frames by include/mdc_jopt.h instead: one Huffman table pair per frame, the file
// libjpeg writes with optimize_coding (PIL: optimize=True) -- the same pixels in smaller files.  The default, huffman=standard, is the
// Annex K tables: today's files byte for byte.
// vignette.png is NOT exported by default, and the exported dataset then opens with validVignette == false, as any dataset without
// that file does.  vignette=1 writes <out>/vignette.png, 16-bit, if the source has a valid vignette (one line says so if not):
//   V = the source's vignetteMap (normalised to a maximum of 1; not the inverse);  R = undistort<float>(V) through the sequence's
//   own UndistorterFOV, on the device like any frame;  m = the maximum of the finite positive R;  every pixel is
//   clamp(rintf(R / m * 65535), 1, 65535), and every pixel whose R is not a finite positive number -- the black border the remap
//   marks with -1, a tap on a zero of the source map -- is 65535.
//   A reader normalises by the maximum and inverts, so the exported map never yields inf or NaN, and a black border pixel, 0 in
//   every frame, stays 0.  GInv[rect(I)] * Vinv_rect approximates rect(GInv[I] * Vinv); it is exact only where the vignette is
//   locally constant.  The quantisation is a one-time table step on the host; the PNG is encoded by mdcp_encode_u16_device.
// The output folder is created if missing; files of these names are overwritten, nothing is deleted.  A frame the reader cannot
// deliver is reported and left out (of images.zip and of times.txt).
#include <sys/stat.h>
#include <sys/types.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "BenchmarkDatasetReader.h"
#include "mdc_hip.h"
#include "mdc_host.h"
#include "mdc_jenc.h"
#include "mdc_jopt.h"
#include "mdc_pnglz.h"
#include "mdc_pngw.h"
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

// The rectified vignette as <out>/vignette.png (the rule is in the header comment).  Returns 0, also when the source has none.
// chain > 0: through include/mdc_pnglz.h with that match depth.
static int export_vignette(DatasetReader* reader, const std::string& dataset, const std::string& out, int w, int h, int chain) {
  mdc_ctx* ctx = reader->getContext();
  const Eigen::Vector2i in = reader->getUndistorter()->getInputDims();
  const size_t n_in = (size_t)in[0] * in[1], n_out = (size_t)w * h;
  mdch_photo* photo = mdch_photo_create((dataset + "pcalib.txt").c_str(), (dataset + "vignette.png").c_str(), in[0], in[1]);
  std::vector<float> map(n_in), rect(n_out, 0.0f);
  const bool valid = photo && (mdch_photo_valid(photo) & 2) && mdch_photo_vignette(photo, map.data(), 0);
  if (photo) mdch_photo_destroy(photo);
  if (!valid) {
    printf("vignette.png: the source has no valid vignette: nothing written\n");
    return 0;
  }
  reader->getUndistorter()->undistort<float>(map.data(), rect.data(), (int)n_in, (int)n_out);
  float top = 0.0f;
  for (size_t i = 0; i < n_out; i++)
    if (std::isfinite(rect[i]) && rect[i] > top) top = rect[i];
  std::vector<uint16_t> q(n_out);
  size_t border = 0;
  for (size_t i = 0; i < n_out; i++) {
    const float r = rect[i];
    if (std::isfinite(r) && r > 0.0f) {
      const float v = rintf(r / top * 65535.0f);
      q[i] = (uint16_t)(v < 1.0f ? 1.0f : v > 65535.0f ? 65535.0f : v);
    } else {
      q[i] = 65535, border++;
    }
  }
  mdcp_encoder* enc = 0;
  mdcl_encoder* lenc = 0;
  uint16_t* d_q = 0;
  uint8_t* d_png = 0;
  int32_t* d_size = 0;
  int64_t slot = 0;
  int32_t size = 0;
  int status = 1;
  std::vector<uint8_t> file;
  if (chain > 0 && (mdcl_create(reader->getDevice(), w, h, MDCL_GRAY16, MDCL_FILTER_ADAPTIVE, chain, 1, &lenc) != MDCL_OK ||
                    mdcl_output_device(lenc, &d_png, &slot, &d_size) != MDCL_OK)) {
    fprintf(stderr, "rectifyDataset: %s\n", mdcl_last_error());
  } else if (chain <= 0 && (mdcp_create(reader->getDevice(), w, h, 16, MDCP_FILTER_ADAPTIVE, 1, &enc) != MDCP_OK ||
                            mdcp_output_device(enc, &d_png, &slot, &d_size) != MDCP_OK)) {
    fprintf(stderr, "rectifyDataset: %s\n", mdcp_last_error());
  } else if (mdc_device_alloc(ctx, n_out * sizeof(uint16_t), (void**)&d_q) != MDC_OK || mdc_copy_to_device(ctx, d_q, q.data(), n_out * sizeof(uint16_t)) != MDC_OK) {
    fprintf(stderr, "rectifyDataset: %s\n", mdc_last_error(ctx));
  } else if (chain > 0 ? mdcl_encode_u16_device(lenc, d_q, (int64_t)n_out, 1, d_png, slot, d_size, 0) != MDCL_OK
                       : mdcp_encode_u16_device(enc, d_q, (int64_t)n_out, 1, d_png, slot, d_size, 0) != MDCP_OK) {
    fprintf(stderr, "rectifyDataset: %s\n", chain > 0 ? mdcl_last_error() : mdcp_last_error());
  } else if (mdc_copy_to_host(ctx, &size, d_size, sizeof size) != MDC_OK || size <= 0 || size > slot ||
             (file.resize((size_t)size), mdc_copy_to_host(ctx, file.data(), d_png, (size_t)size)) != MDC_OK) {
    fprintf(stderr, "rectifyDataset: reading vignette.png back failed: %s\n", mdc_last_error(ctx));
  } else {
    FILE* f = fopen((out + "/vignette.png").c_str(), "wb");
    const bool ok = f && fwrite(file.data(), 1, file.size(), f) == file.size();
    if ((f && fclose(f) != 0) || !ok) fprintf(stderr, "rectifyDataset: cannot write %s/vignette.png\n", out.c_str());
    else status = 0;
  }
  if (d_q) mdc_device_free(ctx, d_q);
  mdcp_destroy(enc);
  mdcl_destroy(lenc);
  if (!status) printf("vignette.png: %d x %d, 16-bit, %d bytes, %zu border pixels at 65535\n", w, h, (int)size, border);
  return status;
}

int main(int argc, char** argv) {
  const char* usage = "usage: %s <dataset folder> <output folder> [quality=95] [frames=jpg|png] [vignette=0|1] [compress=huffman|lz77] [chain=N] [huffman=standard|optimal]\n";
  if (argc < 3) {
    fprintf(stderr, usage, argv[0]);
    return 1;
  }
  std::string dataset = argv[1], out = argv[2];
  int quality = 95;
  bool png = false, vignette = false, lz77 = false, chain_given = false, optimal = false;
  int chain = 4;
  for (int i = 3; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "frames=png" || a == "frames=jpg") png = a == "frames=png";
    else if (a == "vignette=1" || a == "vignette=0") vignette = a == "vignette=1";
    else if (a == "compress=huffman" || a == "compress=lz77") lz77 = a == "compress=lz77";
    else if (a == "huffman=standard" || a == "huffman=optimal") optimal = a == "huffman=optimal";
    else if (a.compare(0, 8, "huffman=") == 0) {
      fprintf(stderr, "rectifyDataset: %s: huffman is standard or optimal\n", argv[i]);
      return 1;
    }
    else if (a.compare(0, 6, "chain=") == 0) {
      char* end = 0;
      const long v = strtol(a.c_str() + 6, &end, 10);
      if (end == a.c_str() + 6 || *end || v < 1 || v > MDCL_MAX_CHAIN) {
        fprintf(stderr, "rectifyDataset: %s: chain is a number 1..%d\n", argv[i], MDCL_MAX_CHAIN);
        return 1;
      }
      chain = (int)v, chain_given = true;
    } else if (a.compare(0, 9, "compress=") == 0) {
      fprintf(stderr, "rectifyDataset: %s: compress is huffman or lz77\n", argv[i]);
      return 1;
    }
    else if (a.compare(0, 8, "quality=") == 0) quality = atoi(a.c_str() + 8);
    else if (a.find('=') == std::string::npos) quality = atoi(argv[i]);
    else {
      fprintf(stderr, "rectifyDataset: unknown argument %s\n", argv[i]);
      fprintf(stderr, usage, argv[0]);
      return 1;
    }
  }
  if (lz77 && !png) {
    fprintf(stderr, "rectifyDataset: compress=lz77 needs frames=png\n");
    return 1;
  }
  if (optimal && png) {
    fprintf(stderr, "rectifyDataset: huffman=optimal needs frames=jpg\n");
    fprintf(stderr, usage, argv[0]);
    return 1;
  }
  if (chain_given && !lz77) {
    fprintf(stderr, "rectifyDataset: chain=%d needs compress=lz77\n", chain);
    return 1;
  }
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
  if (lz77) printf("Rectifying %s: %d frames of %d x %d into %s (PNG, 8-bit, lossless, LZ77 matches of depth %d)\n", dataset.c_str(), total, w, h, out.c_str(), chain);
  else if (png) printf("Rectifying %s: %d frames of %d x %d into %s (PNG, 8-bit, lossless)\n", dataset.c_str(), total, w, h, out.c_str());
  else if (optimal) printf("Rectifying %s: %d frames of %d x %d into %s (JPEG quality %d, optimal Huffman tables)\n", dataset.c_str(), total, w, h, out.c_str(), quality);
  else printf("Rectifying %s: %d frames of %d x %d into %s (JPEG quality %d)\n", dataset.c_str(), total, w, h, out.c_str(), quality);

  const int chunk = total < 128 ? (total > 0 ? total : 1) : 128;
  const size_t frame = (size_t)w * h;
  mdcj_encoder* enc = 0;
  mdcjo_encoder* oenc = 0;
  mdcp_encoder* penc = 0;
  mdcl_encoder* lenc = 0;
  if (lz77 && mdcl_create(reader->getDevice(), w, h, MDCL_GRAY8, MDCL_FILTER_ADAPTIVE, chain, chunk, &lenc) != MDCL_OK) {
    fprintf(stderr, "rectifyDataset: %s\n", mdcl_last_error());
    return 1;
  }
  if (png && !lz77 && mdcp_create(reader->getDevice(), w, h, 8, MDCP_FILTER_ADAPTIVE, chunk, &penc) != MDCP_OK) {
    fprintf(stderr, "rectifyDataset: %s\n", mdcp_last_error());
    return 1;
  }
  if (!png && !optimal && mdcj_create(reader->getDevice(), w, h, quality, chunk, &enc) != MDCJ_OK) {
    fprintf(stderr, "rectifyDataset: %s\n", mdcj_last_error());
    return 1;
  }
  if (optimal && mdcjo_create(reader->getDevice(), w, h, quality, chunk, &oenc) != MDCJO_OK) {
    fprintf(stderr, "rectifyDataset: %s\n", mdcjo_last_error());
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
  if (lz77 ? mdcl_output_device(lenc, &d_out, &slot, &d_sizes) != MDCL_OK
           : png ? mdcp_output_device(penc, &d_out, &slot, &d_sizes) != MDCP_OK
           : optimal ? mdcjo_output_device(oenc, &d_out, &slot, &d_sizes) != MDCJO_OK : mdcj_output_device(enc, &d_out, &slot, &d_sizes) != MDCJ_OK) {
    fprintf(stderr, "rectifyDataset: %s\n", lz77 ? mdcl_last_error() : png ? mdcp_last_error() : optimal ? mdcjo_last_error() : mdcj_last_error());
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
    if (lz77 ? mdcl_encode_f32_device(lenc, d_frames, (int64_t)frame, n, d_out, slot, d_sizes, 0) != MDCL_OK
        : png ? mdcp_encode_f32_device(penc, d_frames, (int64_t)frame, n, d_out, slot, d_sizes, 0) != MDCP_OK
        : optimal ? mdcjo_encode_f32_device(oenc, d_frames, (int64_t)frame, n, d_out, slot, d_sizes, 0) != MDCJO_OK
                  : mdcj_encode_f32_device(enc, d_frames, (int64_t)frame, n, d_out, slot, d_sizes, 0) != MDCJ_OK) {
      fprintf(stderr, "rectifyDataset: %s\n", lz77 ? mdcl_last_error() : png ? mdcp_last_error() : optimal ? mdcjo_last_error() : mdcj_last_error());
      status = 1;
      break;
    }
    if (mdcz_append_device(zip, d_out, slot, d_sizes, valid.data(), n, first, png ? ".png" : ".jpg", 0) != MDCZ_OK) {
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
  mdcjo_destroy(oenc);
  mdcp_destroy(penc);
  mdcl_destroy(lenc);
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
  if (!vignette) printf("vignette.png is not exported (a rectified vignette is out of scope): the dataset opens without a vignette.\n");
  else if (export_vignette(reader, dataset, out, w, h, lz77 ? chain : 0) != 0) status = 1;
  delete reader;
  return status;
}

#include "frame_source.h"

#include <dirent.h>
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>

#include "image_codecs.h"

namespace mdc_host {
namespace {

// name-sorted directory listing, full paths (reference getdir, :44-72)
void list_folder(const std::string& dir, std::vector<std::string>& files) {
  DIR* dp = opendir(dir.c_str());
  if (!dp) return;
  while (struct dirent* e = readdir(dp)) {
    const std::string name = e->d_name;
    if (name != "." && name != "..") files.push_back(name);
  }
  closedir(dp);
  std::sort(files.begin(), files.end());
  for (auto& f : files) f = dir + f;
}

}  // namespace

void FrameSource::open(const std::string& folder) {
  list_folder(folder + "images/", files_);
  if (!files_.empty()) {
    std::printf("Load Dataset %s: found %d files in folder /images; assuming that all images are there.\n", folder.c_str(), (int)files_.size());
    return;
  }
  std::printf("Load Dataset %s: found no in folder /images; assuming that images are zipped.\n", folder.c_str());
  zipped_ = true;
  std::string zerr;
  if (!zip_.open(folder + "images.zip", &zerr)) {
    std::printf("ERROR %d reading archive %s!\n", 1, (folder + "images.zip").c_str());
    std::fprintf(stderr, "DatasetReader: %s\n", zerr.c_str());
    std::exit(1);  // as the reference (:111-115): callers rely on never seeing a reader without frames
  }
  std::vector<std::pair<std::string, int>> named;
  for (int k = 0; k < zip_.entries(); k++) {
    const std::string& n = zip_.name(k);
    if (n == "." || n == "..") continue;
    named.push_back(std::make_pair(n, k));
  }
  std::printf("got %d entries and %d files from zipfile!\n", zip_.entries(), (int)named.size());
  std::sort(named.begin(), named.end());
  for (auto& nk : named) {
    files_.push_back(nk.first);
    zip_index_.push_back(nk.second);
  }
}

bool FrameSource::is_jpeg_name(int id) const {
  const std::string& f = files_[(size_t)id];
  const size_t dot = f.rfind('.');
  if (dot == std::string::npos) return false;
  std::string ext = f.substr(dot + 1);
  for (char& ch : ext) ch = (char)std::tolower((unsigned char)ch);
  return ext == "jpg" || ext == "jpeg";
}

bool FrameSource::read(int id, std::vector<unsigned char>& bytes, std::string* err) const {
  if (zipped_) return zip_.read(zip_index_[(size_t)id], bytes, err);
  if (read_file(files_[(size_t)id], bytes)) return true;
  *err = "cannot read " + files_[(size_t)id];
  return false;
}

}  // namespace mdc_host

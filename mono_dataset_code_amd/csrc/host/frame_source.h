// Where a sequence's frames come from: the name-sorted images/ folder or images.zip (reference
// src/BenchmarkDatasetReader.h:86-125, :256-258).  Listing and "the bytes of frame id"; no threads, no GPU.
// read() is re-entrant: the decode pool calls it from many threads at once.
#pragma once
#include <string>
#include <vector>

#include "zip_reader.h"

namespace mdc_host {

class FrameSource {
 public:
  // Lists `folder`images/, or `folder`images.zip when there is none, and prints the reference's log lines.  An archive that
  // cannot be read ends the process, as the reference does (:111-115).
  void open(const std::string& folder);
  int size() const { return (int)files_.size(); }
  const std::string& name(int id) const { return files_[(size_t)id]; }  // full path (folder) or entry name (zip)
  bool is_jpeg_name(int id) const;
  // Frame id's file, whole; false with *err set when it cannot be read
  bool read(int id, std::vector<unsigned char>& bytes, std::string* err) const;

 private:
  bool zipped_ = false;
  ZipArchive zip_;
  std::vector<std::string> files_;
  std::vector<int> zip_index_;
};

}  // namespace mdc_host

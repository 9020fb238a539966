// The libraries libmdc_host.so loads at run time instead of linking (libmdc_multi.so, the PNG decoders, the lens point libraries):
// one way to find and open them.
#pragma once
#include <dlfcn.h>
#include <cstdlib>
#include <string>

#include "host_device.h"

namespace mdc_host {
// A dlopen handle for `file`, or 0: the path the environment variable `env` holds if `env` is given and set, else `file` in the
// directory libmdc_host.so was loaded from.  The handle is never closed here, and RTLD_NODELETE keeps the library mapped whoever
// closes it: these libraries hold HIP modules (libmdc_multi.so: RCCL's static state and helper threads).
inline void* open_sibling_library(const char* file, const char* env = 0) {
  std::string path;
  const char* named = env ? std::getenv(env) : 0;
  if (named) {
    path = named;
  } else {
    Dl_info info;
    if (dladdr((void*)&open_device_context, &info) && info.dli_fname) {
      path = info.dli_fname;
      const size_t sl = path.rfind('/');
      path = sl == std::string::npos ? std::string() : path.substr(0, sl + 1);
    }
    path += file;
  }
  return dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL | RTLD_NODELETE);
}
}  // namespace mdc_host

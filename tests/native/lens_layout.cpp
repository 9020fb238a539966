// class UndistorterFOV keeps the size and layout it had before it read RadTan / EquiDistant cameras: a program compiled against
// an earlier FOVUndistorter.h allocates that many bytes and runs on today's libmdc_host.so (tests/test_lens_layout_cpu.py).
//
//   lens_layout <camera.txt>...
//
// Each camera is constructed in place in a buffer of exactly the earlier class's size, followed by guard bytes; the program fails
// if the class has grown or if the library wrote a guard byte.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "FOVUndistorter.h"

// the data members of the class before the lens models, in their order
struct EarlierLayout {
  Eigen::Matrix3f k_rect, k_org;
  float calib_in[5], calib_out[5];
  int in_w, in_h, out_w, out_h;
  float* remap_x;
  float* remap_y;
  bool valid;
  void* gpu;
};

int main(int argc, char** argv) {
  static_assert(sizeof(UndistorterFOV) == sizeof(EarlierLayout), "class UndistorterFOV must not grow");
  const size_t size = sizeof(EarlierLayout), guard = 256;
  int bad = 0;
  for (int a = 1; a < argc; a++) {
    unsigned char* p = (unsigned char*)malloc(size + guard);
    if (!p) return 2;
    memset(p, 0xAB, size + guard);
    UndistorterFOV* u = new (p) UndistorterFOV(argv[a]);
    const int kind = u->lensModel();
    const float k0 = u->lensParameters()[0];
    int touched = 0;
    for (size_t i = size; i < size + guard; i++) touched += p[i] != 0xAB;
    fprintf(stderr, "lens_layout: %s: valid %d, lens %d, k[0] %g, %d bytes written past the object's %zu\n", argv[a], (int)u->isValid(), kind, (double)k0,
            touched, size);
    bad += touched != 0;
    u->~UndistorterFOV();
    free(p);
  }
  return bad ? 1 : 0;
}

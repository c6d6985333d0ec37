// thin_face_host.cpp -- the point-triangle routines of hands_amd/csrc/mesh_distance_device.h run on the host, for
// tests/test_thin_faces.py.  Built with the flags of the library (-ffp-contract=off -fno-fast-math) the arithmetic is the
// device's except for 1 / x in place of the reciprocal instruction.
//   thin_face_host IN > OUT
//   IN:  int32 n, int32 P; float32 faces[n][3][3]; float32 queries[n][P][3]      (face i is asked its own P queries)
//   OUT: float32 d2[n][P] of tri_dist2<false>; float32 d2[n][P] and float32 closest[n][P][3] of tri_dist2<true>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "mesh_distance_device.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s IN > OUT\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { perror(argv[1]); return 2; }
  int32_t hdr[2];
  if (fread(hdr, sizeof(int32_t), 2, in) != 2 || hdr[0] < 0 || hdr[1] < 0) { fprintf(stderr, "bad header\n"); return 2; }
  const size_t n = (size_t)hdr[0], P = (size_t)hdr[1];
  std::vector<float> faces(n * 9), q(n * P * 3), d2(n * P), d2p(n * P), cl(n * P * 3);
  if (fread(faces.data(), sizeof(float), faces.size(), in) != faces.size() || fread(q.data(), sizeof(float), q.size(), in) != q.size()) {
    fprintf(stderr, "short file\n");
    return 2;
  }
  fclose(in);
  for (size_t i = 0; i < n; ++i) {
    const float* t = faces.data() + 9 * i;
    const Face f = make_face(t, t + 3, t + 6);
    for (size_t k = 0; k < P; ++k) {
      const size_t o = i * P + k;
      d2[o] = tri_dist2<false>(f, q.data() + 3 * o, nullptr);
      d2p[o] = tri_dist2<true>(f, q.data() + 3 * o, cl.data() + 3 * o);
    }
  }
  const bool ok = fwrite(d2.data(), sizeof(float), d2.size(), stdout) == d2.size() &&
                  fwrite(d2p.data(), sizeof(float), d2p.size(), stdout) == d2p.size() &&
                  fwrite(cl.data(), sizeof(float), cl.size(), stdout) == cl.size();
  return ok && fflush(stdout) == 0 ? 0 : 1;
}

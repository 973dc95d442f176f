// TEST-ONLY: stand-alone driver of the host build of the batched ray tests (pih_rays_emul.cpp), to be compiled with
// -fsanitize=address,undefined and run as a plain program (tests/test_rays.py).  It reads blocks of doubles until the file ends,
//   task (0 peg-in-hole, 1 random-fly), object, flags, n, state record [256 | 48], ray words [n][6]
// with and without the bounding-sphere rejection
// traces every block into a heap buffer of exactly n x 8 words (the rays go through a float buffer of exactly n x 6), and prints the
// number of blocks, rays and hits.
#include "pih_rays_emul.cpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s INPUTS\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  auto rd = [&](size_t n) { std::vector<double> v(n); if (n && fread(v.data(), sizeof(double), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; };
  size_t blocks = 0, total = 0, hits = 0;
  double head[4];
  while (fread(head, sizeof(double), 4, f) == 4) {
    const int task = (int)head[0], object = (int)head[1], flags = (int)head[2], n = (int)head[3];
    if (task < 0 || task > 1 || n < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const std::vector<double> rec = rd(task ? PIH_FLY_STATE_WORDS : PIH_STATE_WORDS), rw = rd((size_t)n * PIH_RAY_WORDS);
    std::vector<float> words(rw.begin(), rw.end());
    std::vector<double> out((size_t)n * PIH_RAY_HIT_WORDS);
    for (int cull = 0; cull < 2; cull++) {
      const int rc = task ? pihray_fly(rec.data(), object, words.data(), n, flags, cull, out.data()) : pihray_view(rec.data(), words.data(), n, flags, cull, out.data());
      if (rc != 0) { fprintf(stderr, "block %zu: rc %d\n", blocks, rc); return 2; }
    }
    for (int r = 0; r < n; r++) hits += out[(size_t)r * PIH_RAY_HIT_WORDS + 1] != (double)PIH_SEG_NONE;
    blocks++; total += (size_t)n;
  }
  fclose(f);
  printf("blocks %zu rays %zu hits %zu\n", blocks, total, hits);
  return 0;
}

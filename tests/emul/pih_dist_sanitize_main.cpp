// TEST-ONLY: stand-alone driver of the host build of the batched closest-point queries (pih_dist_emul.cpp), to be compiled with
// -fsanitize=address,undefined and run as a plain program (tests/test_dist.py).  It reads blocks of doubles until the file ends,
//   task (0 peg-in-hole, 1 random-fly), object, flags, groups, n, state record [256 | 48], query words [n][4]
// answers every block with and without the bounding-sphere rejection into a heap buffer of exactly n x 8 words (the queries go through a
// float buffer of exactly n x 4), and prints the number of blocks, queries and hits.
#include "pih_dist_emul.cpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s INPUTS\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  auto rd = [&](size_t n) { std::vector<double> v(n); if (n && fread(v.data(), sizeof(double), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; };
  size_t blocks = 0, total = 0, hits = 0;
  double head[5];
  while (fread(head, sizeof(double), 5, f) == 5) {
    const int task = (int)head[0], object = (int)head[1], flags = (int)head[2], groups = (int)head[3], n = (int)head[4];
    if (task < 0 || task > 1 || n < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const std::vector<double> rec = rd(task ? PIH_FLY_STATE_WORDS : PIH_STATE_WORDS), qw = rd((size_t)n * PIH_POINT_WORDS);
    std::vector<float> words(qw.begin(), qw.end());
    std::vector<double> out((size_t)n * PIH_CLOSEST_WORDS);
    for (int cull = 0; cull < 2; cull++) {
      const int rc = task ? pihdist_fly(rec.data(), object, words.data(), n, flags, groups, cull, out.data()) : pihdist_view(rec.data(), words.data(), n, flags, groups, cull, out.data());
      if (rc != 0) { fprintf(stderr, "block %zu: rc %d\n", blocks, rc); return 2; }
    }
    for (int r = 0; r < n; r++) hits += out[(size_t)r * PIH_CLOSEST_WORDS + 1] != (double)PIH_SEG_NONE;
    blocks++; total += (size_t)n;
  }
  fclose(f);
  printf("blocks %zu queries %zu hits %zu\n", blocks, total, hits);
  return 0;
}

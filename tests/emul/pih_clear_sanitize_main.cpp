// TEST-ONLY: stand-alone driver of the host build of the robot clearance queries (pih_clear_emul.cpp), to be compiled with
// -fsanitize=address,undefined and run as a plain program (tests/test_clear.py).  It reads blocks of doubles until the file ends,
//   task (0 peg-in-hole, 1 random-fly), object, groups, reach, C (configurations; -1: the record's own joint words), state record [256 | 48],
//   joint words [C][9 | 6]
// answers every block with and without the bounding-sphere rejection into a heap buffer of exactly C x probes x 12 words (the joint words go
// through a float buffer of exactly C x ndof), and prints the number of blocks, records and hits.
#include "pih_clear_emul.cpp"
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
    const int task = (int)head[0], object = (int)head[1], groups = (int)head[2], C = (int)head[4];
    const double reach = head[3];
    if (task < 0 || task > 1 || C < -1) { fprintf(stderr, "bad header\n"); return 2; }
    const int ndof = task ? PIH_UR5_NJ : PIH_ARM_NDOF, np = pihclear_probes(task), n = C < 0 ? 1 : C;
    const std::vector<double> rec = rd(task ? PIH_FLY_STATE_WORDS : PIH_STATE_WORDS), qw = rd(C < 0 ? 0 : (size_t)C * ndof);
    std::vector<float> words(qw.begin(), qw.end());
    std::vector<double> out((size_t)n * np * PIH_CLEAR_WORDS);
    const float* q = C < 0 ? nullptr : words.data();
    for (int cull = 0; cull < 2; cull++) {
      const int rc = task ? pihclear_fly(rec.data(), object, q, n, groups, reach, cull, out.data()) : pihclear_view(rec.data(), q, n, groups, reach, cull, out.data());
      if (rc != 0) { fprintf(stderr, "block %zu: rc %d\n", blocks, rc); return 2; }
    }
    for (size_t r = 0; r < (size_t)n * np; r++) hits += out[r * PIH_CLEAR_WORDS + 1] != (double)PIH_SEG_NONE;
    blocks++; total += (size_t)n * np;
  }
  fclose(f);
  printf("blocks %zu records %zu hits %zu\n", blocks, total, hits);
  return 0;
}

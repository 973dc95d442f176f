// TEST-ONLY: stand-alone driver of the host build of the robot-model queries (pih_robot_emul.cpp), to be compiled with
// -fsanitize=address,undefined and run as a plain program (tests/test_robot_query.py).  It reads the test inputs from a file of doubles
//   robot, n, q[n][ndof], qd[n][ndof], qdd[n][ndof], local[n][3], n_peg, peg states[n_peg][256], n_fly, fly states[n_fly][48]
// runs every query over them (every frame for the Jacobian, with and without local points, with and without qd) into heap buffers of
// exactly the documented sizes, and prints the number of finite output words.
#include "pih_robot_emul.cpp"
#include <cstdio>
#include <vector>

static size_t finite_words(const std::vector<double>& v) { size_t c = 0; for (double x : v) c += (x == x && x - x == 0); return c; }

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s INPUTS\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  auto rd = [&](size_t n) { std::vector<double> v(n); if (n && fread(v.data(), sizeof(double), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; };
  const std::vector<double> head = rd(2);
  const int robot = (int)head[0], n = (int)head[1];
  int d[2];
  if (pihr_dims(robot, d) != 0 || n < 0) { fprintf(stderr, "bad header\n"); return 2; }
  const size_t nd = d[0], nf = d[1];
  const std::vector<double> q = rd(n * nd), qd = rd(n * nd), qdd = rd(n * nd), lp = rd((size_t)n * 3);
  size_t total = 0, fin = 0;
  auto tally = [&](const std::vector<double>& v) { total += v.size(); fin += finite_words(v); };
  { std::vector<double> o(n * nf * LSW); pihr_fk(robot, n, q.data(), qd.data(), o.data()); tally(o); pihr_fk(robot, n, q.data(), nullptr, o.data()); tally(o); }
  for (int frame = 0; frame < (int)nf; frame++) {
    std::vector<double> o(n * 6 * nd);
    pihr_jacobian(robot, n, q.data(), frame, nullptr, o.data()); tally(o);
    pihr_jacobian(robot, n, q.data(), frame, lp.data(), o.data()); tally(o);
  }
  { std::vector<double> o(n * nd * nd); pihr_mass_matrix(robot, n, q.data(), o.data()); tally(o); }
  { std::vector<double> o(n * nd); pihr_inverse_dynamics(robot, n, q.data(), qd.data(), qdd.data(), o.data()); tally(o); }
  const int npeg = (int)rd(1)[0];
  { const std::vector<double> s = rd((size_t)npeg * PIH_STATE_WORDS); std::vector<double> o((size_t)npeg * PEG_FRAMES * LSW);
    pihr_link_states(PIH_TASK_PEG_IN_HOLE, npeg, PIH_STATE_WORDS, s.data(), o.data()); tally(o); }
  const int nfly = (int)rd(1)[0];
  { const std::vector<double> s = rd((size_t)nfly * PIH_FLY_STATE_WORDS); std::vector<double> o((size_t)nfly * FLY_FRAMES * LSW);
    pihr_link_states(PIH_TASK_RANDOM_FLY, nfly, PIH_FLY_STATE_WORDS, s.data(), o.data()); tally(o); }
  fclose(f);
  printf("robot %d n %d words %zu finite %zu\n", robot, n, total, fin);
  return 0;
}

// Host program around csrc/bc_run.h and csrc/bc_batch.h (built with -fsanitize=address,undefined by
// tests/test_run_protocol_cpu.py).  A run's state is given as `null` (no run was ever begun) or as five numbers
// active pending failed done total.  Every command prints one line; `|` separates its fields.
//
//   open <state> <total>                          bc_run_open over that state        -> active pending failed done total
//   admit <name> <noun> <state> <args_ok> <k>     bc_run_admit                       -> rc | message
//   pending <who> <state>                         bc_run_pending                     -> rc | message
//   close <name> <noun> <state>                   bc_run_close                       -> rc | message | was_pending | active pending
//   complete <name> <noun> <state> <was_pending> <none...>   bc_run_complete         -> rc | message
//   walk <who> <cap> <holds> r0 r1 ...            bc_batch_walk over row_ptr         -> rc | largest | message
//   split f0 f1 ...                               bc_batch_unmarked_runs             -> the statuses | the runs as p:q
// The row_ptr and flag arrays are mallocs of exactly their size: a read past them is AddressSanitizer's to see.
#include "../beta_cores_amd/csrc/bc_run.h"
#include "../beta_cores_amd/csrc/bc_batch.h"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static char g_msg[1024] = "";

void bc_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}

// reads a state at argv[*i]; null: the word `null`
static bc_run_state* state_at(char** argv, int argc, int* i, bc_run_state* st) {
  if (*i < argc && !strcmp(argv[*i], "null")) {
    ++*i;
    return nullptr;
  }
  if (*i + 5 > argc) exit(2);
  st->active = atoi(argv[*i]) != 0;
  st->chunk_pending = atoi(argv[*i + 1]) != 0;
  st->failed = atoi(argv[*i + 2]) != 0;
  st->done = atoll(argv[*i + 3]);
  st->total = atoll(argv[*i + 4]);
  *i += 5;
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string cmd = argv[1];
  bc_run_state st;
  int i = 2;
  if (cmd == "open") {
    bc_run_state* r = state_at(argv, argc, &i, &st);
    if (!r || i >= argc) return 2;
    bc_run_open(r, atoll(argv[i]));
    printf("%d %d %d %lld %lld\n", r->active, r->chunk_pending, r->failed, (long long)r->done, (long long)r->total);
    return 0;
  }
  if (cmd == "admit" || cmd == "close" || cmd == "complete") {
    if (argc < 4) return 2;
    const bc_run_kind kd = {argv[2], argv[3]};
    i = 4;
    bc_run_state* r = state_at(argv, argc, &i, &st);
    if (cmd == "admit") {
      if (i + 2 > argc) return 2;
      const int rc = bc_run_admit(r, kd, atoi(argv[i]) != 0, atoi(argv[i + 1]));
      printf("%d|%s\n", rc, g_msg);
    } else if (cmd == "close") {
      bool was = false;
      const int rc = bc_run_close(r, kd, &was);
      printf("%d|%s|%d|%d %d\n", rc, g_msg, was, r ? r->active : 0, r ? r->chunk_pending : 0);
    } else {
      if (!r || i + 2 > argc) return 2;
      const int rc = bc_run_complete(r, kd, atoi(argv[i]) != 0, argv[i + 1]);
      printf("%d|%s\n", rc, g_msg);
    }
    return 0;
  }
  if (cmd == "pending") {
    if (argc < 3) return 2;
    i = 3;
    const int rc = bc_run_pending(state_at(argv, argc, &i, &st), argv[2]);
    printf("%d|%s\n", rc, g_msg);
    return 0;
  }
  if (cmd == "walk") {
    if (argc < 6) return 2;
    const int n = argc - 5;      // row_ptr entries
    int64_t* row_ptr = static_cast<int64_t*>(malloc((size_t)n * sizeof(int64_t)));
    for (int j = 0; j < n; ++j) row_ptr[j] = atoll(argv[5 + j]);
    int64_t largest = -1;
    const int rc = bc_batch_walk(argv[2], row_ptr, n - 1, atoll(argv[3]), argv[4], &largest);
    printf("%d|%lld|%s\n", rc, (long long)largest, g_msg);
    free(row_ptr);
    return 0;
  }
  if (cmd == "split") {
    const size_t P = (size_t)(argc - 2);
    int* flag = static_cast<int*>(malloc(P * sizeof(int)));
    int32_t* status = static_cast<int32_t*>(malloc(P * sizeof(int32_t)));
    for (size_t p = 0; p < P; ++p) {
      flag[p] = atoi(argv[2 + p]);
      status[p] = -7;
    }
    std::vector<std::pair<size_t, size_t>> runs;
    const int rc = bc_batch_unmarked_runs(flag, P, status, [&](size_t p, size_t q) {
      runs.push_back({p, q});
      return BC_OK;
    });
    if (rc != BC_OK) return 1;
    for (size_t p = 0; p < P; ++p) printf("%s%d", p ? " " : "", status[p]);
    printf("|");
    for (size_t k = 0; k < runs.size(); ++k) printf("%s%zu:%zu", k ? " " : "", runs[k].first, runs[k].second);
    printf("\n");
    free(flag);
    free(status);
    return 0;
  }
  return 2;
}

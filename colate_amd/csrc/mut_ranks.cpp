// colate_amd/csrc/mut_ranks.cpp -- `Colate --mode mut --ranks N` (rank_ctx.h): the rank context, the communicator of the ranks and
// the launcher that forks them, relays the communicator id and reaps them.
#include <fcntl.h>
#include <poll.h>
#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "cli_lists.h"
#include "cli_modes.h"
#include "colate_amd.h"
#include "colate_internal.h"
#include "rank_ctx.h"

namespace colate_drv {

RankCtx g_rank;

static bool write_all(int fd, const void* buf, size_t n) {
  const char* p = static_cast<const char*>(buf);
  while (n) {
    ssize_t k = ::write(fd, p, n);
    if (k <= 0) return false;
    p += k, n -= (size_t)k;
  }
  return true;
}
static bool read_all(int fd, void* buf, size_t n) {
  char* p = static_cast<char*>(buf);
  while (n) {
    ssize_t k = ::read(fd, p, n);
    if (k <= 0) return false;
    p += k, n -= (size_t)k;
  }
  return true;
}

bool RankComm::open(const Options& opt) {
#ifdef COLATE_TEST_HOOKS  // (only in lib/testhooks/libcolate_amd.so, which the tests of the launcher load: never in the product library)
  if (const char* h = std::getenv("COLATE_TEST_HANG_RANK")) {  // a rank stuck as if inside a collective
    if (std::atoi(h) == g_rank.rank)
      for (;;) ::pause();
  }
#endif
  const int ndev = colate_device_count();
  if (ndev < 1) {
    std::cerr << "Error: " << colate_last_error() << std::endl;
    return false;
  }
  const int dev0 = opt.has("device") ? opt.get_int("device") : 0;
  unsigned char id[COLATE_COMM_ID_BYTES];
  int rc = colate_set_device((dev0 + g_rank.rank) % ndev);
  if (!rc) {
    if (g_rank.rank == 0) {
      rc = colate_comm_unique_id(id);
      if (!write_all(g_rank.fd_id_out, id, rc ? 0 : sizeof(id)) && !rc) rc = COLATE_EIO;
      ::close(g_rank.fd_id_out);  // (on failure the launcher sees end-of-file and tells the others)
    } else if (!read_all(g_rank.fd_id_in, id, sizeof(id))) {
      std::cerr << "Error: rank " << g_rank.rank << " did not receive the communicator id." << std::endl;
      return false;
    }
  }
  if (!rc) rc = colate_comm_create(id, g_rank.nranks, g_rank.rank, &comm);
  if (rc) api_error(rc);
  return !rc;
}

// `--ranks N`: fork N processes BEFORE anything touches the GPU (this process never does), one per GPU; each runs the
// whole `--mode mut` pipeline (same inputs, same --seed, hence the same tables and bootstrap weights), computes its
// contiguous range of replicates and takes part in one RCCL all-gather (colate_comm.cpp); rank 0 writes the outputs.
// The launcher only relays rank 0's 128-byte communicator id to the other ranks and collects the exit codes.
int run_ranked(const Options& opt, int nranks) {
  if (colate_device_touched()) {
    // fork() after the HIP runtime is up gives children with a half-copied runtime (its threads and device queues are
    // not duplicated): they hang or fault.  The command-line `Colate` never gets here; a host process that has already
    // computed through this library (or that shares it with torch) must start the ranks as fresh processes instead.
    std::cerr << "Error: --ranks forks one process per GPU and must run before this process first uses a GPU through "
                 "libcolate_amd; start `Colate --ranks N` as its own process (never re-exec from here)." << std::endl;
    return 1;
  }
  if (!opt.has("seed")) {
    std::cerr << "Error: --ranks needs --seed (every rank must draw the same bootstrap weights)." << std::endl;
    return 1;
  }
  // (--ranks is always given here: the refused option the sentence names is --ranks, and what it ends with is --devices)
  if (opt.has("devices") && refuse_options(opt, {"ranks"}, "--devices")) return 1;
  if (opt.has("pairs") && opt.has("counts_out") && !opt.has("counts_only")) {
    // (the ranks all-gather the rates, not the counts; --counts_only computes every pair's counts on rank 0)
    std::cerr << "Error: --ranks cannot write the .counts files of a --pairs list (--counts_out) unless --counts_only is given."
              << std::endl;
    return 1;
  }
  // where the ranks other than 0 keep their progress lines: next to the output (with --pairs: next to the list of pairs)
  const std::string log_prefix = opt.has("pairs") ? opt.get("pairs") : opt.get("output");
  int up[2];
  if (::pipe(up) != 0) {
    std::perror("pipe");
    return 1;
  }
  std::vector<int> down_r(nranks, -1), down_w(nranks, -1);
  for (int r = 1; r < nranks; r++) {
    int fd[2];
    if (::pipe(fd) != 0) {
      std::perror("pipe");
      return 1;
    }
    down_r[r] = fd[0], down_w[r] = fd[1];
  }
  std::cerr.flush();
  std::cout.flush();
  std::vector<pid_t> pids(nranks, -1);
  for (int r = 0; r < nranks; r++) {
    pid_t pid = ::fork();
    if (pid < 0) {
      std::perror("fork");
      return 1;
    }
    if (pid == 0) {  // rank r
      g_rank.ranked = true, g_rank.rank = r, g_rank.nranks = nranks;
      ::close(up[0]);
      for (int q = 1; q < nranks; q++) {
        ::close(down_w[q]);
        if (q != r) ::close(down_r[q]);
      }
      if (r == 0) {
        g_rank.fd_id_out = up[1];
      } else {
        ::close(up[1]);
        g_rank.fd_id_in = down_r[r];
        // only rank 0 talks on the terminal; the others keep their progress lines in a file that a clean exit removes
        const std::string log = log_prefix + ".rank" + std::to_string(r) + ".stderr";
        if (!std::freopen(log.c_str(), "w", stderr)) std::perror("freopen");
      }
      int code = 1;
      try {
        code = opt.has("pairs") ? run_mut_pairs(opt) : run_mut(opt);
      } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << std::endl;
      }
      std::cerr.flush();
      if (r != 0 && code == 0) std::remove((log_prefix + ".rank" + std::to_string(r) + ".stderr").c_str());
      std::fflush(nullptr);
      ::_exit(code);
    }
    pids[r] = pid;
  }
  ::close(up[1]);
  for (int r = 1; r < nranks; r++) ::close(down_r[r]);
  // One loop relays rank 0's communicator id to the other ranks AND reaps the ranks as they end (our own pids only: this
  // function is also reachable through the library ABI, whose host may have children of its own).  Nothing here blocks:
  //  * a rank that fails before or outside the collective leaves the others waiting in ncclCommInitRank / ncclAllGather
  //    for ever, so the first failure -- or any exit while the id is still outstanding -- starts a grace period
  //    (COLATE_RANK_GRACE_SEC, default 15 s: ranks that are merely finishing get there) after which the rest are killed;
  //  * rank 0 ending without having published the id closes the other ranks' pipes (they report and exit);
  //  * a rank 0 that neither publishes the id nor ends (stuck in HIP initialisation, ncclGetUniqueId or its table fill)
  //    is given COLATE_RANK_ID_TIMEOUT_SEC (default 3600 s: the id follows the table fill, which may be long), then
  //    every rank is killed and the launcher returns non-zero.
  double grace_s = 15.0, id_timeout_s = 3600.0;
  if (const char* g = std::getenv("COLATE_RANK_GRACE_SEC")) grace_s = std::atof(g);
  if (const char* g = std::getenv("COLATE_RANK_ID_TIMEOUT_SEC")) id_timeout_s = std::atof(g);
  unsigned char id[COLATE_COMM_ID_BYTES];
  size_t id_have = 0;
  bool id_open = true;
  auto close_id_pipes = [&]() {
    if (!id_open) return;
    ::close(up[0]);
    for (int r = 1; r < nranks; r++) ::close(down_w[r]);
    id_open = false;
  };
  ::fcntl(up[0], F_SETFL, ::fcntl(up[0], F_GETFL, 0) | O_NONBLOCK);
  const auto t_start = std::chrono::steady_clock::now();
  auto seconds_since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
  };
  int worst = 0, remaining = nranks;
  std::vector<char> done(nranks, 0);
  bool failing = false, killed = false;
  auto t_fail = std::chrono::steady_clock::now();
  auto kill_rest = [&]() {
    for (int r = 0; r < nranks; r++)
      if (!done[r]) ::kill(pids[r], SIGKILL);
    killed = true;
  };
  while (remaining > 0) {
    bool progressed = false;
    if (id_open) {  // (waits up to 20 ms for bytes of the id: this is also the loop's pause)
      pollfd pfd{up[0], POLLIN, 0};
      if (::poll(&pfd, 1, 20) > 0) {
        const ssize_t k = ::read(up[0], id + id_have, sizeof(id) - id_have);
        if (k > 0) {
          id_have += (size_t)k;
          if (id_have == sizeof(id)) {
            for (int r = 1; r < nranks; r++) write_all(down_w[r], id, sizeof(id));
            close_id_pipes();
          }
          progressed = true;
        } else if (k == 0) {  // rank 0 ended (or closed its end) without an id: end-of-file for the others, too
          close_id_pipes();
        }
      }
      if (id_open && !killed && seconds_since(t_start) > id_timeout_s) {
        std::cerr << "Error: rank 0 has not published the communicator id after " << id_timeout_s
                  << " s (COLATE_RANK_ID_TIMEOUT_SEC); ending all ranks." << std::endl;
        close_id_pipes();
        kill_rest();
        worst = 1;
      }
    }
    for (int r = 0; r < nranks; r++) {
      if (done[r]) continue;
      int st = 0;
      const pid_t w = ::waitpid(pids[r], &st, WNOHANG);
      if (w == 0) continue;
      done[r] = 1, remaining--, progressed = true;
      const bool ok = (w == pids[r]) && WIFEXITED(st) && WEXITSTATUS(st) == 0;
      if (!ok) {
        std::cerr << "Error: rank " << r << (killed ? " was ended by the launcher" : " failed");
        if (r > 0) std::cerr << " (see " << log_prefix << ".rank" << r << ".stderr)";
        std::cerr << std::endl;
        worst = 1;
      }
      // a failure -- or any exit while the id is outstanding (nobody can finish properly without it) -- starts the clock
      if ((!ok || (id_open && nranks > 1)) && !failing) failing = true, t_fail = std::chrono::steady_clock::now();
    }
    if (remaining == 0) break;
    if (failing && !killed && seconds_since(t_fail) > grace_s) {
      std::cerr << "Error: a rank failed; ending the " << remaining << " rank(s) still waiting after " << grace_s << " s."
                << std::endl;
      close_id_pipes();
      kill_rest();
      worst = 1;
    }
    if (!progressed && !id_open) ::usleep(20000);
  }
  close_id_pipes();
  return worst;
}

}  // namespace colate_drv

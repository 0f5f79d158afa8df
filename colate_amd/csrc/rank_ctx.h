// colate_amd/csrc/rank_ctx.h -- `Colate --mode mut --ranks N` (mut_ranks.cpp): the launcher that forks one process per GPU, what a
// rank knows about itself, and the RCCL communicator the ranks gather their results over.
#pragma once
#include "cli_options.h"
#include "colate_amd.h"

namespace colate_drv {

// `--ranks N`: this process is rank `rank` of `nranks` (run_ranked forks them); the 128-byte RCCL id travels from
// rank 0 to the others through the launcher's pipes.
struct RankCtx {
  bool ranked = false;  // launched by run_ranked (also with one rank: the RCCL path with a communicator of one)
  int rank = 0, nranks = 1;
  int fd_id_out = -1;  // rank 0: writes the id here
  int fd_id_in = -1;   // ranks > 0: read it here
};
extern RankCtx g_rank;

// `--ranks`: this rank's GPU, (--device + rank) % the node's devices, and the RCCL communicator of all ranks, whose id rank 0
// creates and the launcher relays (run_ranked).  The communicator is destroyed with the object.
struct RankComm {
  void* comm = nullptr;
  RankComm() = default;
  RankComm(const RankComm&) = delete;
  RankComm& operator=(const RankComm&) = delete;
  ~RankComm() { colate_comm_destroy(comm); }

  bool open(const Options& opt);  // false after the error message
};

// Runs the mode as `nranks` ranks and returns the worst exit code (the comment at its definition: what it relays and reaps).
int run_ranked(const Options& opt, int nranks);

}  // namespace colate_drv

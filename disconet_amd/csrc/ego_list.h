// Who is in an ego's list (upstream DiscoNet.forward's loops; include/disconet_hip.h states it per entry point): the ego i,
// then the live j != i ascending, skipping j when only_v2i && i != 0 && j != 0 (vehicles talk to the infrastructure,
// agent 0, only).  A padded ego (i >= the live count) has a list of one.  Every kernel that walks or builds a list
// takes the rule from here and keeps its own way of storing it.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace {

// scene b's live agents 0 .. n - 1: a bad count never indexes past the agents
__device__ inline int live_count(const int32_t* num_agent, int b, int agents) {
  const int n = num_agent[b];
  return n < 0 ? 0 : (n > agents ? agents : n);
}

// may i and j exchange maps at all: under only_v2i a vehicle (i != 0) talks to the infrastructure, agent 0, only
#define DN_V2I_PAIR(i, j, only_v2i) (!(only_v2i) || (i) == 0 || (j) == 0)

// is j behind i in LIVE ego i's list (i and j below the live count: a loop over the live j of an ego that is no padding).
// A macro: as an inlined function the same expression makes the compiler build the callers' list loops differently
// (peeled, more registers), and dn_agent_fuse and dn_late_fuse measured slower for it.
#define DN_LISTED_LIVE(i, j, only_v2i) ((j) != (i) && DN_V2I_PAIR(i, j, only_v2i))

// the same for any pair of agents: nobody is listed behind a padded ego, a dead j in no list
__device__ inline bool listed(int i, int j, int n_live, int only_v2i) {
  return j != i && i < n_live && j < n_live && DN_V2I_PAIR(i, j, only_v2i);
}

}  // namespace

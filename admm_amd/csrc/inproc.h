// In-process multi-device mode of admm_hip_parlasso / admm_hip_parbp (PAR_DEVICES): the ranks of one call are threads of the
// calling process, one per listed device, joined by an in-process PEER group (comm.h).
#pragma once
#include "admm_internal.h"
#include <functional>

namespace admm {

// rank r runs on devices[r] for r < the largest divisor of nblocks that is <= the number of listed devices (whole blocks per rank);
// empty when that is one rank: the single-device path
std::vector<int> par_layout(int nblocks, const std::vector<int>& listed);
std::vector<int> par_devices_for(int nblocks);                      // ... for the devices the PAR_DEVICES option lists
// the device that holds the caller's device input, -1 for host input
int input_device(const void* x, int mem);

// Runs body(rank, nranks) on one thread per rank, rank r on devices[r], as the ranks of an in-process PEER group.  The caller's
// thread options go with every rank; a device that holds more than one rank takes the two-launch PEER form (several ranks' launches
// must never depend on being resident together).  src_device >= 0: the caller's input lives on that device -- every rank device
// must reach it over peer access.  Throws the first failing rank's error (a rank's own failure before another's ADMM_ERR_COMM).
void run_inproc(const std::vector<int>& devices, int src_device, const std::function<void(int, int)>& body);

// admm_hip_last_parallel_layout: the devices of the calling thread's last parallel call (empty: no call yet)
const std::vector<int>& last_layout();
void record_single_layout();

}  // namespace admm

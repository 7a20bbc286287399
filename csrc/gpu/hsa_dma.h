// hsa_dma.h — the HSA pieces shared by the two SDMA copy paths (engine.hip: device -> host
// fetch, ingest.hip: file -> HBM): the CPU agent, the blocking signal wait and an owning
// completion signal.
#pragma once

#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <cstdint>

namespace tv {
namespace gpu {

// the CPU agent (the host end of an SDMA copy), found once; handle 0: none
inline hsa_agent_t hsa_cpu_agent() {
  static const hsa_agent_t a = [] {
    hsa_agent_t r{0};
    hsa_iterate_agents(
        [](hsa_agent_t x, void* data) {
          hsa_device_type_t t;
          if (hsa_agent_get_info(x, HSA_AGENT_INFO_DEVICE, &t) == HSA_STATUS_SUCCESS && t == HSA_DEVICE_TYPE_CPU) {
            *static_cast<hsa_agent_t*>(data) = x;
            return HSA_STATUS_INFO_BREAK;
          }
          return HSA_STATUS_SUCCESS;
        },
        &r);
    return r;
  }();
  return a;
}

// Owns one completion signal.  A copy queued on it counts it down by one; wait() blocks until
// it is below 1.  The destructor waits before it destroys, so the signal never goes away
// under a copy in flight: whoever gives up on copies that were counted but never queued must
// take them off first (drop()).
class HsaSignal {
 public:
  explicit HsaSignal(hsa_signal_value_t initial) {
    if (hsa_signal_create(initial, 0, nullptr, &s_) != HSA_STATUS_SUCCESS) s_.handle = 0;
  }
  HsaSignal(HsaSignal&& o) noexcept : s_(o.s_) { o.s_.handle = 0; }
  HsaSignal(const HsaSignal&) = delete;
  HsaSignal& operator=(const HsaSignal&) = delete;
  ~HsaSignal() {
    if (!ok()) return;
    wait();
    hsa_signal_destroy(s_);
  }
  bool ok() const { return s_.handle != 0; }  // false: hsa_signal_create failed
  hsa_signal_t get() const { return s_; }
  void set(hsa_signal_value_t v) const { hsa_signal_store_relaxed(s_, v); }
  void drop(hsa_signal_value_t n) const { hsa_signal_subtract_screlease(s_, n); }
  void wait() const {
    while (hsa_signal_wait_scacquire(s_, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED) >= 1) {
    }
  }

 private:
  hsa_signal_t s_{0};
};

}  // namespace gpu
}  // namespace tv

// stage_scratch.hpp -- the owner of a coder stage's device blocks: a list of the stage's pointers and the device they were
// allocated on.  The blocks exist all or not at all, a stage is used on the device that holds them, and they go back to
// the cache (devmem.cpp) with the stage.  Host code, free of hip_runtime.h like common.hpp.
#pragma once
#include "common.hpp"

namespace ifhip {

// a stage is used on the device its blocks were allocated on
inline int stage_on_device(int stage_device, int current_device) {
    if (current_device == stage_device) return IFHIP_OK;
    return fail(IFHIP_INVALID_STATE, "InvalidState: stage belongs to device %d, current device is %d", stage_device, current_device);
}

class StageScratch {
  public:
    // The stage's pointers (null until the blocks exist); they outlive the owner: declare it behind them.  A typed pointer is
    // read and cleared through void** here, as DEV_MALLOC fills it: every object pointer has one representation on this target.
    template <typename... T>
    explicit StageScratch(T**... blocks) : blocks_{reinterpret_cast<void**>(blocks)...} { static_assert(sizeof...(T) <= 16, "blocks_ holds 16"); }
    StageScratch(const StageScratch&) = delete;      // (it points into the stage that holds it)
    ~StageScratch() { release(); }

    bool allocated() const { return device_ >= 0; }
    // The current device must be a gfx950 and, once the blocks exist, the one that holds them.
    int check_device(int* device_out = nullptr) const {
        int dev = -1;
        if (int rc = require_gfx950(&dev)) return rc;
        if (device_out) *device_out = dev;
        return allocated() ? stage_on_device(device_, dev) : IFHIP_OK;
    }
    // The first call allocates on the current device: allocate_all() fills every pointer, one HIP_TRY(DEV_MALLOC(..)) each, and returns
    // IFHIP_OK or the status of the one that failed -- then what it took is freed and the stage is as it was.  Later calls only check the device.
    template <typename AllocateAll>
    int ensure(AllocateAll allocate_all) {
        int dev = -1;
        if (int rc = check_device(&dev)) return rc;
        if (allocated()) return IFHIP_OK;
        if (int rc = allocate_all()) { release(); return rc; }
        device_ = dev;
        return IFHIP_OK;
    }

  private:
    void release() { for (void** p : blocks_) if (p) { (void)cached_free(*p); *p = nullptr; } }    // (device_ is still -1 where a stage lives on)
    void** const blocks_[16];       // (the rest is null)
    int device_ = -1;
};

}  // namespace ifhip

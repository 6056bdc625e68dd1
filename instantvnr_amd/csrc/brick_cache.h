// brick_cache.h — the inference cache of a network: the de-hashed brick image (grid_levels.h), the level table that points into it, and the
// policy that says when it exists (brick_policy.h).  Network holds one and asks it, before every evaluation launch, which level table to pass.
#pragma once

#include "brick_policy.h"
#include "common.h"

namespace vnr {

class BrickCache {
public:
  // what an image is built from: the network's level table (host), its parameter blob's grid part and the plain level table (device)
  struct Source {
    const LevelInfo* levels;
    uint32_t n_levels, n_features;
    const uint16_t* table;
    const LevelInfo* levels_dev;
  };

  ~BrickCache();
  // The level table of a launch of capacity `n_max` enqueued on `s`, and the image it reads (null: `source.levels_dev`, the parameter blob).
  // Builds the image first when the policy says so: on `s`, returning only after the host has seen the build complete, so launches on any
  // stream may read it (a per-launch hipStreamWaitEvent on the build's event stood here: one more API call and one more barrier packet in
  // front of every evaluation kernel, always on a completed event)
  const LevelInfo* levels_for_launch(const Source& source, hipStream_t s, const uint8_t** image, size_t n_max);
  void parameters_changed() { policy_.parameters_changed(); }
  // -1: the environment's policy (VNR_AMD_BRICK, default automatic: built once VNR_AMD_BRICK_AFTER launches, default 24 = two frames of the
  // streaming renderer, have seen unchanged parameters), 0: never (drops an existing image), 1: build at the next launch
  void set_mode(int mode);
  // budget of the image in bytes (0: the default, VNR_AMD_BRICK_MAX_GB or else 1/16 of the device's memory); drops an existing image, which
  // is rebuilt within the new budget, and within a quarter of the free device memory, by the next launches
  void set_budget(size_t bytes);
  // Levels finer than `cap` grid points per axis are left hashed: the image pays off where neighbouring samples share cells,
  // i.e. up to about the resolution of the volume the network represents (NeuralVolume passes twice its largest dimension).
  // A 128^3 volume with tcnn's default per_level_scale 2 has levels up to 2048^3, whose image would be 137 GB and useless.
  void set_resolution_cap(uint32_t cap) { res_cap_ = cap; }
  // idles the device and gives the image's memory back; the next launches read the parameter blob until the policy builds another
  void drop();

  size_t bytes() const { return image_.bytes(); }
  bool in_use() const { return policy_.tier != BrickPolicy::kNone; }
  uint32_t levels_mask() const { return mask_; }   // bit l: level l is read from the image
  float build_ms() const { return build_ms_; }
  const BrickPolicy& policy() const { return policy_; }
  uint32_t after_now() const;   // launches with unchanged parameters the next full build waits for

private:
  void build(const Source& source, hipStream_t s, BrickPolicy::Tier tier);

  DeviceBuffer<uint8_t> image_{MemTag::Network};
  DeviceBuffer<LevelInfo> levels_{MemTag::Network};   // the plan's level table
  BrickPolicy policy_;
  hipEvent_t t0_ = nullptr, t1_ = nullptr;   // around a build: created by the first one
  float build_ms_ = 0.0f;
  uint32_t mask_ = 0;
  uint32_t res_cap_ = 0;   // 0: no cap
  size_t budget_ = 0;      // 0: default policy
};

}  // namespace vnr

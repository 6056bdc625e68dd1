// network_host.hip — host side of the network engine: model JSON -> layout, parameter blob handling,
// (de)serialisation in tcnn's Trainer::serialize format, launch wrappers.
//
// Reference: core/networks/tcnn_network.h:157-272; EXTERNAL tiny-cuda-nn (GridEncodingTemplated ctor,
// FullyFusedMLP, Trainer::serialize/deserialize) — assumptions listed in SURVEY.md Appendix A.
#include "network.h"

#include <algorithm>
#include <cstdlib>
#include <set>

#include "infer_kernel.h"

namespace vnr {

void launch_pack_mlp(const uint16_t* params, uint16_t* packed, uint16_t* packedT, uint32_t in_width, uint32_t W, uint32_t n_hidden_matmuls, hipStream_t s);
void launch_fused(int mode, const GridDevice& grid, uint32_t in_width, const FusedMlp& mlp, const LevelInfo* d_levels, const uint16_t* table, size_t table_bytes,
                  const float* coords, float* out, uint16_t* features_out, uint16_t* acts_out, size_t n, const uint32_t* d_n, size_t n_max, hipStream_t s,
                  const uint32_t* d_dest = nullptr, uint32_t queue_out_stride = 0, const uint8_t* brick_image = nullptr,
                  uint32_t sharers = 1, const struct PackArgs* pack = nullptr);
void launch_init_params(OptState* state, uint16_t* params, size_t n_mlp, size_t n_total, uint32_t in_width,
                        uint32_t n_hidden_matmuls, uint32_t width, uint64_t seed, hipStream_t s);
// master weights <- fp16 parameters; reset_optimizer also zeroes the moments and step counts
void launch_master_from_f16(const uint16_t* params, OptState* state, size_t n, bool reset_optimizer, hipStream_t s);

// ------------------------------------------------------------------------------------------------
uint16_t f32_to_f16(float f)
{
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  const uint32_t ax = x & 0x7fffffffu;
  if (ax >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | ((ax > 0x7f800000u) ? (0x200u | ((ax >> 13) & 0x3ffu)) : 0u));
  if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);
  if (ax < 0x33000001u) return (uint16_t)sign;
  const int32_t e = (int32_t)(ax >> 23) - 127;
  const uint32_t m = (ax & 0x7fffffu) | 0x800000u;
  const uint32_t shift = e < -14 ? (uint32_t)(-1 - e) : 13u;
  const uint32_t he = e < -14 ? 0u : (uint32_t)(e + 15);
  uint32_t q = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (q & 1u))) q++;
  return (uint16_t)(sign | (he == 0 ? q : ((he - 1) << 10) + q));
}

float f16_to_f32(uint16_t h)
{
  const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  uint32_t x;
  if (e == 0) {
    if (m == 0) x = sign;
    else { float v = (float)m * 5.9604644775390625e-8f; std::memcpy(&x, &v, 4); x |= sign; }
  } else if (e == 31) x = sign | 0x7f800000u | (m << 13);
  else x = sign | ((e + 112u) << 23) | (m << 13);
  float f;
  std::memcpy(&f, &x, 4);
  return f;
}

// EXTERNAL tcnn GridEncodingTemplated ctor (level sizing) + grid_index's hash decision; scale/resolution
// as used by core/networks/tcnn_impl_decoder.cu:41-42.
uint32_t grid_make_layout(const ModelConfig& cfg, GridDevice* out)
{
  if (cfg.n_levels > (uint32_t)kMaxLevels) throw std::runtime_error("too many hash-grid levels");
  const float log2_pls = std::log2(cfg.per_level_scale);
  uint32_t offset = 0;
  for (uint32_t l = 0; l < cfg.n_levels; ++l) {
    const float scale = exp2f((float)l * log2_pls) * (float)cfg.base_resolution - 1.0f;
    const uint32_t res = (uint32_t)ceilf(scale) + 1u;
    const uint32_t max_params = 0xffffffffu / 2u;
    const double cube = (double)res * (double)res * (double)res;
    uint32_t n = cube > (double)max_params ? max_params : (uint32_t)cube;
    n = next_multiple(n, 8u);
    // EXTERNAL tcnn GridEncodingTemplated ctor: Dense keeps the full level, Tiled caps it at base_resolution^3 (the level then repeats
    // with that period), Hash at 2^log2_hashmap_size
    if (cfg.grid_type == 2u) {
      const double tile = (double)cfg.base_resolution * cfg.base_resolution * cfg.base_resolution;
      if ((double)n > tile) n = (uint32_t)tile;
    } else if (cfg.grid_type == 0u) {
      const uint32_t cap = 1u << cfg.log2_hashmap_size;
      if (n > cap) n = cap;
    }
    if (n == 0) throw std::runtime_error("grid level without entries");
    // tcnn grid_index: the stride walk stops as soon as the stride exceeds the level's size; a Hash grid then hashes instead
    uint32_t stride = 1, dims = 0;
    for (; dims < 3 && stride <= n; ++dims) stride *= res;
    LevelInfo& lv = out->levels[l];
    lv.scale = scale;
    lv.resolution = res;
    lv.res2 = res * res;
    lv.size = n;
    lv.offset = offset;
    if (cfg.grid_type == 0u) lv.hashed = n < stride ? 1u : 0u;
    else lv.hashed = (dims == 3 && (uint64_t)res * res * res <= (uint64_t)n) ? 0u : 1u + dims;   // 2 / 3 / 4: index over 1 / 2 / 3 dimensions, modulo
    lv.brick = lv.pad1 = 0;
    if (lv.hashed == 1u && (n & (n - 1)) != 0) throw std::runtime_error("internal: hashed level with non power-of-two size");
    if ((uint64_t)offset + n > 0xffffffffull) throw std::runtime_error("grid encoding too large (more than 2^32 entries)");
    offset += n;
  }
  out->n_levels = cfg.n_levels;
  out->n_features = cfg.n_features;
  out->interpolation = cfg.interpolation;
  return offset;
}

static std::set<Network*>& live_networks()
{
  static std::set<Network*> s;
  return s;
}

static uint32_t json_u32(const Json& j, const char* key, uint32_t def) { return j.contains(key) ? (uint32_t)j.at(key).as_int() : def; }
static float json_f32(const Json& j, const char* key, float def) { return j.contains(key) ? j.at(key).as_float() : def; }
static std::string json_str(const Json& j, const char* key, const char* def) { return j.contains(key) ? j.at(key).as_string() : std::string(def); }

void Network::configure(const Json& config, uint64_t init_seed)
{
  // tcnn_network.h:167-175: only loss / encoding / network are kept in the serialised model; the optimizer
  // options persist across re-configuration (m_optimizer_opts).
  const Json loss = config.value("loss", Json::object());
  const Json enc = config.value("encoding", Json::object());
  const Json net = config.value("network", Json::object());
  ModelConfig c = cfg_;  // keeps previous optimizer options unless given
  if (config.contains("optimizer")) {
    const Json& opt = config.at("optimizer");
    const std::string ot = json_str(opt, "otype", "Adam");
    const Json* adam = &opt;
    if (ot == "ExponentialDecay") {
      c.has_decay = true;
      c.decay_start = json_u32(opt, "decay_start", 10000);
      c.decay_interval = json_u32(opt, "decay_interval", 10000);  // tcnn defaults
      c.decay_base = json_f32(opt, "decay_base", 0.33f);
      if (!opt.contains("nested")) throw std::runtime_error("ExponentialDecay optimizer needs a 'nested' optimizer");
      adam = &opt.at("nested");
    } else {
      c.has_decay = false;
    }
    if (json_str(*adam, "otype", "Adam") != "Adam") throw std::runtime_error("unsupported optimizer otype (Adam / ExponentialDecay{Adam} only)");
    c.learning_rate = json_f32(*adam, "learning_rate", 1e-3f);
    c.beta1 = json_f32(*adam, "beta1", 0.9f);
    c.beta2 = json_f32(*adam, "beta2", 0.999f);
    c.epsilon = json_f32(*adam, "epsilon", 1e-8f);
    c.l2_reg = json_f32(*adam, "l2_reg", 1e-8f);
  }
  const std::string lt = json_str(loss, "otype", "L2");
  if (lt == "L1") c.loss = 0;
  else if (lt == "L2") c.loss = 1;
  else throw std::runtime_error("unsupported loss otype: " + lt);

  const std::string et = json_str(enc, "otype", "");
  // EXTERNAL tcnn create_grid_encoding: otype Grid / HashGrid / TiledGrid / DenseGrid, "type" (default by otype) Hash / Dense / Tiled
  if (et != "HashGrid" && et != "Grid" && et != "DenseGrid" && et != "TiledGrid")
    throw std::runtime_error("unsupported encoding otype: '" + et + "' (HashGrid / Grid / DenseGrid / TiledGrid)");
  const std::string gt = json_str(enc, "type", et == "DenseGrid" ? "Dense" : et == "TiledGrid" ? "Tiled" : "Hash");
  if (gt == "Hash") c.grid_type = 0;
  else if (gt == "Dense") c.grid_type = 1;
  else if (gt == "Tiled") c.grid_type = 2;
  else throw std::runtime_error("unsupported grid type: " + gt + " (Hash / Dense / Tiled)");
  c.n_levels = json_u32(enc, "n_levels", 16);
  c.n_features = json_u32(enc, "n_features_per_level", 2);
  c.log2_hashmap_size = json_u32(enc, "log2_hashmap_size", 19);
  c.base_resolution = json_u32(enc, "base_resolution", 16);
  c.per_level_scale = json_f32(enc, "per_level_scale", 2.0f);
  const std::string it = json_str(enc, "interpolation", "Linear");
  if (it == "Linear") c.interpolation = 0;
  else if (it == "Smoothstep") c.interpolation = 1;
  else if (it == "Nearest") c.interpolation = 2;
  else throw std::runtime_error("unsupported interpolation: " + it);
  // the reference reads both from the tcnn encoding object (tcnn_device_api.h:53-54), where only tcnn's own API can set them, so
  // a params.json never carries them; here they may be given with the encoding (absent = tcnn's defaults)
  c.quantize_threshold = json_f32(enc, "quantize_threshold", 0.0f);
  c.max_level = json_f32(enc, "max_level", 1000.0f);
  if (c.n_features != 1 && c.n_features != 2 && c.n_features != 4 && c.n_features != 8)
    throw std::runtime_error("n_features_per_level must be 1, 2, 4 or 8");  // method_raymarching.cu:1241-1244
  if (c.log2_hashmap_size > 28) throw std::runtime_error("log2_hashmap_size too large");

  const std::string nt = json_str(net, "otype", "FullyFusedMLP");
  if (nt != "FullyFusedMLP") throw std::runtime_error("unsupported network otype: " + nt + " (FullyFusedMLP only)");
  c.n_neurons = json_u32(net, "n_neurons", 128);
  c.n_hidden_layers = json_u32(net, "n_hidden_layers", 5);
  if (c.n_neurons != 16 && c.n_neurons != 32 && c.n_neurons != 64 && c.n_neurons != 128)
    throw std::runtime_error("FullyFusedMLP n_neurons must be 16, 32, 64 or 128");   // tcnn_impl.cu:315-347
  if (c.n_hidden_layers < 1) throw std::runtime_error("n_hidden_layers must be >= 1");
  // the activations the reference's kernels dispatch (tcnn_impl.cu:405-415, tcnn_device_api.h:274-285; no Sine there)
  auto activation_of = [](const std::string& a, const char* what) -> uint32_t {
    if (a == "None") return kActNone;
    if (a == "ReLU") return kActReLU;
    if (a == "Exponential") return kActExponential;
    if (a == "Sigmoid") return kActSigmoid;
    if (a == "Squareplus") return kActSquareplus;
    if (a == "Softplus") return kActSoftplus;
    throw std::runtime_error(std::string("unsupported ") + what + ": " + a + " (None / ReLU / Exponential / Sigmoid / Squareplus / Softplus)");
  };
  c.activation = activation_of(json_str(net, "activation", "ReLU"), "activation");
  c.output_activation = activation_of(json_str(net, "output_activation", "None"), "output_activation");

  cfg_ = c;
  model_ = Json::object();
  model_["loss"] = loss;
  model_["encoding"] = enc;
  model_["network"] = net;
  build_layout();
  steps_ = 0;
  lr_ = cfg_.learning_rate;   // a re-configured model starts its schedule over (tcnn_network.h:195-209 rebuilds optimizer and trainer)
  initialize_params(init_seed, Runtime::get().stream);
  live_networks().insert(this);
}

void Network::build_layout()
{
  const uint32_t total_entries = grid_make_layout(cfg_, &grid_);
  in_width_ = next_multiple(cfg_.n_levels * cfg_.n_features, 16u);
  // the instances of the fused kernel (infer_kernel.h dispatch): refuse the others here, at SetModel, not at the first launch
  const uint32_t widest = cfg_.n_features == 1 ? 32u : cfg_.n_features == 2 ? 64u : 128u;   // (1 and 2 features: all of kMaxLevels = 32 levels)
  if (in_width_ > widest)
    throw std::runtime_error("unsupported encoding shape: n_features_per_level=" + std::to_string(cfg_.n_features) + " with n_levels=" +
                             std::to_string(cfg_.n_levels) + " (encoded width " + std::to_string(in_width_) + " > " + std::to_string(widest) + ")");
  const size_t W = cfg_.n_neurons;
  n_mlp_ = W * in_width_ + (size_t)n_hidden_matmuls() * W * W + (size_t)16 * W;
  n_params_ = n_mlp_ + (size_t)total_entries * cfg_.n_features;
  if ((n_params_ - n_mlp_) * sizeof(uint16_t) >= (1ull << 32)) throw std::runtime_error("hash table >= 4 GiB is not supported");
  lds_halves_ = packed_mlp_halves(in_width_, cfg_.n_neurons, n_hidden_matmuls());
  lds_halves_T_ = packedT_halves(in_width_, cfg_.n_neurons, n_hidden_matmuls());
  params_f16_.resize(n_params_);
  mlp_packed_.resize(lds_halves_);
  mlp_packed_T_.resize(lds_halves_T_);
  levels_dev_.resize(kMaxLevels);
  levels_dev_.upload(grid_.levels, kMaxLevels, Runtime::get().stream);
  VNR_HIP_CHECK(hipStreamSynchronize(Runtime::get().stream));
  // training state is allocated lazily on the first training step
  opt_state_.release(); grads_.release(); grads_f32_.release();
  ws_batch_ = 0;
}

void Network::initialize_params(uint64_t seed, hipStream_t s)
{
  opt_state_.resize(n_params_);
  launch_init_params(opt_state_.ptr, params_f16_.ptr, n_mlp_, n_params_, in_width_, n_hidden_matmuls(), cfg_.n_neurons, seed, s);
  ++params_generation_;
  opt_sharded_ = false;
  refresh_inference_weights(s);
}

uint32_t Network::n_active_levels() const
{
  uint32_t n = 0;
  while (n < cfg_.n_levels && !((float)n >= cfg_.max_level + 1e-3f)) ++n;
  return n;
}

void Network::refresh_inference_weights(hipStream_t s)
{
  // both weight images (forward; transposed for the MLP backward) in one launch
  launch_pack_mlp(params_f16_.ptr, mlp_packed_.ptr, mlp_packed_T_.ptr, in_width_, cfg_.n_neurons, n_hidden_matmuls(), s);
  // the parameters changed: the brick image is stale (it is rebuilt once they have been left alone again -- for longer if this image was
  // dropped before it had paid for itself: brick_policy.h)
  brick_.parameters_changed();
}

Network::~Network()
{
  live_networks().erase(this);
  for (hipEvent_t e : prof_events_) (void)hipEventDestroy(e);
  if (side_stream_) { (void)hipStreamSynchronize(side_stream_); (void)hipStreamDestroy(side_stream_); (void)hipEventDestroy(ev_fork_); (void)hipEventDestroy(ev_join_); }
}

void Network::set_train_profiling(bool e)
{
  train_profiling_ = e;
  prof_steps_ = 0;
  if (e && prof_events_.empty()) {
    prof_events_.resize((size_t)kTrainProfileSteps * (kTrainPhases + 1));
    for (hipEvent_t& ev : prof_events_) VNR_HIP_CHECK(hipEventCreate(&ev));
  }
}

void Network::profile_mark(int boundary, hipStream_t s)
{
  if (!train_profiling_) return;
  VNR_HIP_CHECK(hipEventRecord(prof_events_[(size_t)(prof_steps_ % kTrainProfileSteps) * (kTrainPhases + 1) + boundary], s));
  if (boundary == kTrainPhases) ++prof_steps_;
}

int Network::train_profile(double* ms_per_step)
{
  for (int p = 0; p < kTrainPhases; ++p) ms_per_step[p] = 0.0;
  const int n = (int)std::min<uint64_t>(prof_steps_, kTrainProfileSteps);
  if (!train_profiling_ || n == 0) return 0;
  VNR_HIP_CHECK(hipEventSynchronize(prof_events_[(size_t)((prof_steps_ - 1) % kTrainProfileSteps) * (kTrainPhases + 1) + kTrainPhases]));
  for (int k = 0; k < n; ++k)
    for (int p = 0; p < kTrainPhases; ++p) {
      float ms = 0.0f;
      VNR_HIP_CHECK(hipEventElapsedTime(&ms, prof_events_[(size_t)k * (kTrainPhases + 1) + p], prof_events_[(size_t)k * (kTrainPhases + 1) + p + 1]));
      ms_per_step[p] += ms / n;
    }
  return n;
}

void Network::release_temporary()
{
  brick_.drop();   // (idles the device: nothing may still read what is freed, here or below)
  ws_features_.release(); ws_acts_.release(); ws_dfeat_.release();   // re-allocated by the next training step (ws_batch_ = 0)
  ws_batch_ = 0;
}

void Network::release_temporary_of_all()
{
  for (Network* n : live_networks()) n->release_temporary();
}

void Network::set_params_f16(const uint16_t* host, size_t count, hipStream_t s)
{
  if (count != n_params_) throw std::runtime_error("parameter count mismatch: got " + std::to_string(count) + ", model has " + std::to_string(n_params_));
  VNR_HIP_CHECK(hipMemcpyAsync(params_f16_.ptr, host, count * sizeof(uint16_t), hipMemcpyHostToDevice, s));
  if (opt_state_.count == n_params_) launch_master_from_f16(params_f16_.ptr, opt_state_.ptr, n_params_, false, s);  // moments kept, as before
  ++params_generation_;
  refresh_inference_weights(s);
  VNR_HIP_CHECK(hipStreamSynchronize(s));
}

void Network::get_params_f16(uint16_t* host, size_t count, hipStream_t s) const
{
  if (count != n_params_) throw std::runtime_error("parameter count mismatch");
  VNR_HIP_CHECK(hipMemcpyAsync(host, params_f16_.ptr, count * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
  VNR_HIP_CHECK(hipStreamSynchronize(s));
}

// EXTERNAL tcnn Trainer::serialize(): {"n_params", "params_type": "__half", "params_binary"} (key names
// confirmed by apps/view_model.cpp:124-126); no optimizer state with the reference's default arguments.
Json Network::serialize_params(hipStream_t s) const
{
  std::vector<uint16_t> host(n_params_);
  get_params_f16(host.data(), n_params_, s);
  Json j = Json::object();
  j["n_params"] = (uint64_t)n_params_;
  j["params_type"] = "__half";
  j["params_binary"] = Json::binary(host.data(), host.size() * sizeof(uint16_t));
  return j;
}

void Network::deserialize_params(const Json& j, hipStream_t s)
{
  const size_t n = (size_t)j.at("n_params").as_int();
  if (n != n_params_) throw std::runtime_error("Can't set params because buffer has the wrong size: " + std::to_string(n) + " vs " + std::to_string(n_params_));
  const std::string type = j.at("params_type").as_string();
  const std::string& bin = j.at("params_binary").as_binary();
  std::vector<uint16_t> host(n);
  if (type == "__half") {
    if (bin.size() != n * 2) throw std::runtime_error("params_binary has the wrong size");
    std::memcpy(host.data(), bin.data(), n * 2);
  } else if (type == "float") {
    if (bin.size() != n * 4) throw std::runtime_error("params_binary has the wrong size");
    const float* f = (const float*)bin.data();
    for (size_t i = 0; i < n; ++i) host[i] = f32_to_f16(f[i]);
  } else {
    throw std::runtime_error("Unknown params_type: " + type);
  }
  set_params_f16(host.data(), n, s);
  if (j.contains("optimizer") || j.contains("step")) { /* optimizer state is not stored by the reference */ }
}

void Network::inference(const float* d_coords, float* d_out, size_t n, const uint32_t* d_n, size_t n_max, hipStream_t s,
                        const uint32_t* d_dest) const
{
  const uint8_t* image;
  const LevelInfo* levels = brick_.levels_for_launch(brick_source(), s, &image, d_n ? n_max : n);
  GridDevice grid = grid_;
  grid.n_levels = n_active_levels();   // masked levels encode to zero, like the padding
  launch_fused(0, grid, in_width_, fused_mlp(), levels, params_f16_.ptr + n_mlp_, n_grid_params() * 2, d_coords, d_out, nullptr, nullptr, n, d_n, n_max, s, d_dest, 0, image);
}

bool Network::inference_queue(const float* d_records, float* d_out, uint32_t out_stride, const uint32_t* d_n, size_t n_max, hipStream_t s,
                              uint32_t sharers, const PackArgs* pack) const
{
  const uint8_t* image;
  const LevelInfo* levels = brick_.levels_for_launch(brick_source(), s, &image, n_max);
  GridDevice grid = grid_;
  grid.n_levels = n_active_levels();
  if (cfg_.n_neurons == 128u) pack = nullptr;   // blocks of 8 waves: the caller launches the packing kernel itself
  launch_fused(0, grid, in_width_, fused_mlp(), levels, params_f16_.ptr + n_mlp_, n_grid_params() * 2, d_records, d_out, nullptr, nullptr, 0, d_n, n_max, s, nullptr,
               out_stride, image, sharers, pack);
  return pack != nullptr;
}

FusedMlp Network::fused_mlp() const
{
  const bool wglobal = !weights_in_lds();   // the A operands from global memory: a model whose weights do not fit the LDS
  return FusedMlp{mlp_packed_.ptr, lds_halves_, cfg_.n_neurons, n_hidden_matmuls(), cfg_.activation, cfg_.output_activation, !common_kind() || wglobal, wglobal,
                  cfg_.quantize_threshold};
}

bool Network::tile_net(TileNet* out, hipStream_t s) const
{
  if (!weights_in_lds()) return false;   // (a deeper network reads its weights from global memory: evaluation kernels only)
  if (n_grid_params() * 2 >= (1ull << 32)) throw std::runtime_error("hash table >= 4 GiB is not supported");
  const uint8_t* image;
  const LevelInfo* levels = brick_.levels_for_launch(brick_source(), s, &image, BrickPolicy::kSmallMinLaunch);   // (a frame evaluated inside the marching / tracking loop)
  out->levels = levels;
  out->n_levels = n_active_levels();
  out->interpolation = grid_.interpolation;
  out->table = (const half_t*)(params_f16_.ptr + n_mlp_);
  out->table_bytes = (uint32_t)(n_grid_params() * 2);
  out->brick_image = image;
  out->packed_mlp = (const half_t*)mlp_packed_.ptr;
  out->lds_halves = lds_halves_;
  out->n_hidden_matmuls = n_hidden_matmuls();
  out->activation = cfg_.activation;
  out->output_activation = cfg_.output_activation;
  out->n_features = grid_.n_features;
  out->in_width = in_width_;
  out->width = cfg_.n_neurons;
  out->general = common_kind() ? 0u : 1u;
  out->quantize_threshold = cfg_.quantize_threshold;
  return true;
}

void Network::encode(const float* d_coords, uint16_t* d_features, size_t n, hipStream_t s) const
{
  const uint8_t* image;
  const LevelInfo* levels = brick_.levels_for_launch(brick_source(), s, &image, n);
  GridDevice grid = grid_;
  grid.n_levels = n_active_levels();
  launch_fused(1, grid, in_width_, fused_mlp(), levels, params_f16_.ptr + n_mlp_, n_grid_params() * 2, d_coords, nullptr, d_features, nullptr, n, nullptr, n, s, nullptr, 0, image);
}

size_t Network::bytes_allocated() const
{
  return brick_.bytes() + params_f16_.bytes() + mlp_packed_.bytes() + mlp_packed_T_.bytes() + opt_state_.bytes() + grads_.bytes() + grads_f32_.bytes() + ws_features_.bytes() + ws_acts_.bytes() + ws_dfeat_.bytes() + ws_loss_.bytes();
}

}  // namespace vnr

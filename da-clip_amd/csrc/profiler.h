// profiler.h — the in-engine conv profiler behind dac_profile_*: one record per timed launch and
// the state of the pass that made them. ProfileLog is host-only (no HIP header, like pack.h;
// tools/profiler_check.cpp tests it alone, DAC_PROFILER_HOST_ONLY); Profiler adds the device
// side: the event pairs of an eager pass, the stamp buffer of a stamped one.
#pragma once
#include <cstdio>
#include <string>
#include <vector>

#include "error.h"

namespace dac {

struct Launch {
  int cls = 0;                   // conv class (kh*100 + conv_variant; 350 = the fused ResBlock)
  double flops = 0, bytes = 0;   // algorithmic work
  double ms = 0;                 // measured duration
  double t0_ms = -1;             // stamped pass: start, ms after the replay's first timed launch
  bool in_branch = false;        // launched inside a concurrent branch of the UNet's split section
  std::string label, symbol;     // shape label; stamped pass: kernel symbol(s), '+'-joined
};

// What the last pass was. counting: the dry run that counts the launches to time; events: the
// eager replay with a HIP event pair around each; stamps: the captured loop graph, every timed
// launch writing [begin, end] wall-clock stamps (StampGuard, common.h), replayed once.
enum class Pass { none, counting, events, stamps };

constexpr int kStampSlots = 64;  // [begin, end] pairs per launch (= STAMP_SLOTS, common.h)

// The argument struct a kernel takes by value as its first parameter, by the kernel's own name
// (`name` mangled or demangled, template arguments or not); none for every kernel not listed.
enum class KernArgs { none, conv, rb };
KernArgs symbol_args(const std::string& name);

struct ProfileLog {
  static constexpr int ALL = 999;            // kernel_id: every conv launch, labelled by shape
  int kernel_id = -1;                        // conv class to time, -1 = off
  bool stamps = false;                       // dac_profile_mode: what the NEXT pass will be
  Pass pass = Pass::none;                    // what the records came from
  bool have_ms = false;                      // durations read out (reduce_stamps / finish_events)
  size_t counted = 0;                        // launches the counting pass saw
  double graph_ms = 0;                       // stamped pass: HIP-event time of the replay
  std::vector<Launch> rec;

  bool on() const { return kernel_id >= 0; }
  bool wants(int cls) const { return kernel_id == ALL || kernel_id == cls; }
  void begin_pass(Pass p) { pass = p; have_ms = false; counted = 0; graph_ms = 0; rec.clear(); }
  void enable(int id) { kernel_id = id; begin_pass(Pass::none); }
  // After the live recording: it timed exactly the launches the counting pass saw.
  void check_complete() const;
  // Durations and start times from a stamped replay's stamps [n][kStampSlots][2] (khz = the
  // wall clock's rate): min begin .. max end over the slots a block wrote (the others still hold
  // [~0, 0]), starts relative to the earliest begin. DAC_E_STATE for a launch without stamps.
  void reduce_stamps(const unsigned long long* host_stamps, size_t n, int khz);
  struct Summary { int n; double mean_ms, flops_per_launch, bytes_per_launch; };
  Summary summary() const;                   // DAC_E_STATE: nothing profiled
  void report(FILE* f) const;                // DAC_PROFILE_PRINT: time and TFLOP/s per label
  const Launch& at(int i) const;             // DAC_E_ARG: out of range or durations not read
};

}  // namespace dac

#ifndef DAC_PROFILER_HOST_ONLY
#include <hip/hip_runtime.h>

namespace dac {

struct Profiler : ProfileLog {
  Profiler() = default;
  Profiler(const Profiler&) = delete;
  ~Profiler();
  // After the counting pass: events or initialised stamp slots for `counted` launches; the pass
  // becomes events or stamps (by `stamps`).
  void prepare(hipStream_t st);
  // Around one timed launch. begin returns the launch's stamp block (null in an eager pass);
  // DAC_E_STATE for a launch prepare did not cover.
  unsigned long long* begin(hipStream_t st);
  void end(hipStream_t st, Launch&& l);
  void finish_events();                      // eager pass: waits, reads every pair's elapsed time
  // Stamped pass: each record's symbol from the captured graph's kernel nodes (the stamp pointer
  // in a listed kernel's argument struct names the launch), then one replay between two events.
  void name_symbols(hipGraph_t g, hipStream_t st);
  void finish_stamps(hipGraphExec_t ex, hipStream_t st, int device);

 private:
  std::vector<hipEvent_t> ev;                // begin / end pairs, and one to bracket the replay
  unsigned long long* sbuf = nullptr;
  size_t scap = 0;                           // launches sbuf holds
};

}  // namespace dac
#endif

// profiler.cpp — see profiler.h. The host-only part first, the device side after it.
#include "profiler.h"

#include <algorithm>
#include <cctype>
#include <map>

namespace dac {

// The kernel's own name: the last <length><name> of a mangled symbol's scope, or what stands
// before the template / parameter list of a demangled one, without its scope.
static std::string kernel_base(const std::string& s) {
  if (s.rfind("_Z", 0) == 0) {
    size_t i = s.compare(2, 1, "N") == 0 ? 3 : 2;
    std::string base;
    while (i < s.size() && isdigit((unsigned char)s[i])) {
      size_t n = 0;
      while (i < s.size() && isdigit((unsigned char)s[i]) && n <= s.size()) n = 10 * n + (s[i++] - '0');
      if (n > s.size() - i) return "";
      base = s.substr(i, n);
      i += n;
    }
    return base;
  }
  const std::string b = s.substr(0, s.find_first_of("<("));
  const size_t c = b.find_last_of(": ");
  return c == std::string::npos ? b : b.substr(c + 1);
}

KernArgs symbol_args(const std::string& name) {
  // Every kernel that constructs a StampGuard from its argument struct's stamp, and the split-K
  // reduction, which receives its conv's ConvArgs (same stamp pointer) and so joins its symbol.
  static const struct { const char* base; KernArgs args; } table[] = {
      {"conv_kernel", KernArgs::conv},   {"conv2_kernel", KernArgs::conv},  {"conv3_kernel", KernArgs::conv},
      {"conv3i_kernel", KernArgs::conv}, {"conv3w_kernel", KernArgs::conv}, {"conv_down_kernel", KernArgs::conv},
      {"conv7_kernel", KernArgs::conv},  {"conv3n_kernel", KernArgs::conv}, {"conv8_kernel", KernArgs::conv},
      {"conv3q_kernel", KernArgs::conv}, {"conv3r_kernel", KernArgs::conv}, {"rbfuse_kernel", KernArgs::rb},
      {"conv_part_reduce_kernel", KernArgs::conv}};
  const std::string base = kernel_base(name);
  for (const auto& e : table)
    if (base == e.base) return e.args;
  return KernArgs::none;
}

void ProfileLog::check_complete() const {
  if (rec.size() != counted) throw Error(DAC_E_STATE, "profiler: dry and live recordings differ");
}

void ProfileLog::reduce_stamps(const unsigned long long* hs, size_t n, int khz) {
  if (n != rec.size() || khz <= 0) throw Error(DAC_E_STATE, "profiler: stamps do not match the records");
  unsigned long long origin = ~0ull;
  std::vector<unsigned long long> begin(n);
  for (size_t i = 0; i < n; ++i) {
    unsigned long long b0 = ~0ull, b1 = 0;
    for (int k = 0; k < kStampSlots; ++k) {                // slots no block used stay [max, 0]
      b0 = std::min(b0, hs[2 * (kStampSlots * i + k)]);
      b1 = std::max(b1, hs[2 * (kStampSlots * i + k) + 1]);
    }
    if (b0 == ~0ull || b1 < b0)
      throw Error(DAC_E_STATE, "profile_graph: launch " + std::to_string(i) + " left no stamps");
    rec[i].ms = (double)(b1 - b0) / (double)khz;           // ticks / kHz = ms
    begin[i] = b0;
    origin = std::min(origin, b0);
  }
  for (size_t i = 0; i < n; ++i) rec[i].t0_ms = ((double)begin[i] - (double)origin) / (double)khz;
  have_ms = true;
}

ProfileLog::Summary ProfileLog::summary() const {
  if (!on() || rec.empty() || pass == Pass::none || pass == Pass::counting)
    throw Error(DAC_E_STATE, "nothing profiled");
  if (!have_ms) throw Error(DAC_E_STATE, "graph profile incomplete");
  double ms = 0, fl = 0, by = 0;
  for (const Launch& l : rec) { ms += l.ms; fl += l.flops; by += l.bytes; }
  const int n = (int)rec.size();
  return {n, ms / n, fl / n, by / n};
}

void ProfileLog::report(FILE* f) const {
  struct Row { double n = 0, ms = 0, flops = 0; };
  std::map<std::string, Row> by;
  double tot = 0;
  for (const Launch& l : rec) {
    Row& r = by[l.label];
    r.n += 1; r.ms += l.ms; r.flops += l.flops;
    tot += l.ms;
  }
  std::vector<std::pair<double, std::string>> rows;
  for (const auto& kv : by) {
    char line[320];
    snprintf(line, sizeof line, "%6.0f x %8.1f us = %8.2f ms  %7.1f TF/s  %s", kv.second.n,
             1e3 * kv.second.ms / kv.second.n, kv.second.ms, kv.second.flops / (kv.second.ms * 1e-3) / 1e12,
             kv.first.c_str());
    rows.push_back({kv.second.ms, line});
  }
  std::sort(rows.rbegin(), rows.rend());
  fprintf(f, "[dac conv profile] %zu launches, %.2f ms total\n", rec.size(), tot);
  for (const auto& r : rows) fprintf(f, "  %s\n", r.second.c_str());
}

const Launch& ProfileLog::at(int i) const {
  if (i < 0 || (size_t)i >= rec.size() || !have_ms)
    throw Error(DAC_E_ARG, "dac_profile_launch: index out of range (call dac_profile_read first)");
  return rec[i];
}

}  // namespace dac

#ifndef DAC_PROFILER_HOST_ONLY
#include "common.h"
#include "kernels.h"

namespace dac {

static_assert(kStampSlots == STAMP_SLOTS, "profiler.h and common.h disagree on the stamp slots");

Profiler::~Profiler() {
  for (auto e : ev) (void)hipEventDestroy(e);
  if (sbuf) (void)hipFree(sbuf);
}

void Profiler::prepare(hipStream_t st) {
  const size_t n = counted;
  begin_pass(stamps ? Pass::stamps : Pass::events);
  counted = n;
  // Pairs for n launches (eager pass) and one more, which brackets the stamped replay.
  while (ev.size() < 2 * (n + 1)) {
    hipEvent_t e;
    HIP_OK(hipEventCreate(&e));
    ev.push_back(e);
  }
  if (pass != Pass::stamps) return;
  if (n > scap) {
    if (sbuf) HIP_OK(hipFree(sbuf));
    sbuf = nullptr;
    scap = 0;
    HIP_OK(hipMalloc(&sbuf, 2 * kStampSlots * n * sizeof(unsigned long long)));
    scap = n;
  }
  stamp_init(sbuf, (size_t)kStampSlots * n, st);
}

unsigned long long* Profiler::begin(hipStream_t st) {
  const size_t i = rec.size();
  if ((pass != Pass::events && pass != Pass::stamps) || i >= counted)
    throw Error(DAC_E_STATE, "profiler: launch " + std::to_string(i) + " was not counted by the dry pass");
  if (pass == Pass::stamps) return sbuf + 2 * kStampSlots * i;
  HIP_OK(hipEventRecord(ev[2 * i], st));
  return nullptr;
}

void Profiler::end(hipStream_t st, Launch&& l) {
  if (pass == Pass::events) HIP_OK(hipEventRecord(ev[2 * rec.size() + 1], st));
  rec.push_back(std::move(l));
}

void Profiler::finish_events() {
  for (size_t i = 0; i < rec.size(); ++i) {
    HIP_OK(hipEventSynchronize(ev[2 * i + 1]));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
    rec[i].ms = ms;
  }
  have_ms = true;
}

void Profiler::name_symbols(hipGraph_t g, hipStream_t st) {
  const size_t n = rec.size();
  size_t nn = 0;
  if (hipGraphGetNodes(g, nullptr, &nn) != hipSuccess || !nn) return;
  std::vector<hipGraphNode_t> nodes(nn);
  if (hipGraphGetNodes(g, nodes.data(), &nn) != hipSuccess) return;
  for (size_t i = 0; i < nn; ++i) {
    hipGraphNodeType ty;
    if (hipGraphNodeGetType(nodes[i], &ty) != hipSuccess || ty != hipGraphNodeTypeKernel) continue;
    hipKernelNodeParams kp{};
    if (hipGraphKernelNodeGetParams(nodes[i], &kp) != hipSuccess || !kp.func || !kp.kernelParams || !kp.kernelParams[0])
      continue;
    const char* nm = hipKernelNameRefByPtr(kp.func, st);
    if (!nm) continue;
    const KernArgs ka = symbol_args(nm);
    if (ka == KernArgs::none) continue;
    unsigned long long* sp = ka == KernArgs::rb ? static_cast<const RbArgs*>(kp.kernelParams[0])->stamp
                                                : static_cast<const ConvArgs*>(kp.kernelParams[0])->stamp;
    if (!sp || sp < sbuf || sp >= sbuf + 2 * kStampSlots * n) continue;
    std::string& dst = rec[(size_t)(sp - sbuf) / (2 * kStampSlots)].symbol;
    dst = dst.empty() ? nm : dst + "+" + nm;
  }
}

void Profiler::finish_stamps(hipGraphExec_t ex, hipStream_t st, int device) {
  const size_t n = rec.size();
  hipEvent_t e0 = ev[2 * n], e1 = ev[2 * n + 1];
  HIP_OK(hipEventRecord(e0, st));
  HIP_OK(hipGraphLaunch(ex, st));
  HIP_OK(hipEventRecord(e1, st));
  HIP_OK(hipEventSynchronize(e1));
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  graph_ms = ms;
  std::vector<unsigned long long> hs(2 * kStampSlots * n);
  HIP_OK(hipMemcpy(hs.data(), sbuf, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  int khz = 0;
  HIP_OK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device));
  if (khz <= 0) throw Error(DAC_E_HIP, "profile_graph: no wall-clock rate");
  reduce_stamps(hs.data(), n, khz);
}

}  // namespace dac
#endif

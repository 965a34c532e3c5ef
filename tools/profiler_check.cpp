// profiler_check.cpp — host-only check of the profiler's HIP-free part (csrc/profiler.h,
// ProfileLog and symbol_args) on synthetic data: `make -C da-clip_amd profcheck` builds it with
// -DDAC_PROFILER_HOST_ONLY under AddressSanitizer + UBSan; tests/test_profiler.py runs it.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../da-clip_amd/csrc/profiler.h"

using namespace dac;

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// f() throws a dac::Error with this code whose message contains `text`.
template <class F>
static bool throws(int code, const char* text, F&& f) {
  try {
    f();
  } catch (const Error& e) {
    return e.code == code && strstr(e.what(), text);
  }
  return false;
}

using Stamps = std::vector<unsigned long long>;
static Stamps blank(size_t n) {
  Stamps s(2 * kStampSlots * n);
  for (size_t i = 0; i < s.size(); i += 2) { s[i] = ~0ull; s[i + 1] = 0; }
  return s;
}
static void put(Stamps& s, size_t launch, int slot, unsigned long long b, unsigned long long e) {
  s[2 * (kStampSlots * launch + slot)] = b;
  s[2 * (kStampSlots * launch + slot) + 1] = e;
}

static ProfileLog three_records(Pass pass) {
  ProfileLog p;
  p.enable(ProfileLog::ALL);
  p.begin_pass(pass);
  p.rec.push_back({312, 6e9, 3e6, 0.0, -1.0, false, "c312 a", ""});
  p.rec.push_back({350, 2e9, 1e6, 0.0, -1.0, true, "c350 b", "rbfuse_kernel"});
  p.rec.push_back({312, 1e9, 5e6, 0.0, -1.0, true, "c312 a", "conv3_kernel+conv_part_reduce_kernel"});
  return p;
}

static void check_reduce() {
  const int khz = 100000;
  ProfileLog p = three_records(Pass::stamps);
  Stamps s = blank(3);
  // launch 0: all 64 slots; begins 5000 + 7k (min 5000), ends 9000 + 11k (max 9693)
  for (int k = 0; k < kStampSlots; ++k) put(s, 0, (k * 5) % kStampSlots, 5000 + 7 * k, 9000 + 11 * k);
  // launch 1: three slots, the rest blank; it holds the global origin 1000
  put(s, 1, 2, 1500, 2500);
  put(s, 1, 40, 1000, 2200);
  put(s, 1, 63, 1200, 4000);
  // launch 2: one slot
  put(s, 2, 17, 123456789000ull, 123456989000ull);
  p.reduce_stamps(s.data(), 3, khz);
  CHECK(p.have_ms);
  CHECK(p.rec[0].ms == (9693.0 - 5000.0) / 100000.0 && p.rec[0].t0_ms == (5000.0 - 1000.0) / 100000.0);
  CHECK(p.rec[1].ms == (4000.0 - 1000.0) / 100000.0 && p.rec[1].t0_ms == 0.0);
  CHECK(p.rec[2].ms == 200000.0 / 100000.0 && p.rec[2].t0_ms == (123456789000.0 - 1000.0) / 100000.0);

  ProfileLog q = three_records(Pass::stamps);
  Stamps t = s;
  for (int k = 0; k < kStampSlots; ++k) put(t, 2, k, ~0ull, 0);                  // launch 2 wrote nothing
  CHECK(throws(DAC_E_STATE, "launch 2 left no stamps", [&] { q.reduce_stamps(t.data(), 3, khz); }));
  t = s;
  put(t, 1, 2, ~0ull, 0);
  put(t, 1, 63, ~0ull, 0);
  put(t, 1, 40, 1000, 900);                                                      // max end below min begin
  CHECK(throws(DAC_E_STATE, "launch 1 left no stamps", [&] { q.reduce_stamps(t.data(), 3, khz); }));
  CHECK(throws(DAC_E_STATE, "", [&] { q.reduce_stamps(s.data(), 2, khz); }));    // not one block per record
}

static void check_at_summary_report() {
  ProfileLog p = three_records(Pass::events);
  CHECK(throws(DAC_E_ARG, "out of range", [&] { p.at(0); }));                    // durations not read yet
  p.rec[0].ms = 0.5; p.rec[1].ms = 0.25; p.rec[2].ms = 1.5;
  p.rec[1].t0_ms = 0.125;
  p.have_ms = true;
  CHECK(throws(DAC_E_ARG, "out of range", [&] { p.at(-1); }));
  CHECK(throws(DAC_E_ARG, "out of range", [&] { p.at(3); }));
  const Launch& l = p.at(1);
  CHECK(l.cls == 350 && l.flops == 2e9 && l.bytes == 1e6 && l.ms == 0.25 && l.t0_ms == 0.125 && l.in_branch &&
        l.label == "c350 b" && l.symbol == "rbfuse_kernel");
  CHECK(p.at(2).symbol == "conv3_kernel+conv_part_reduce_kernel" && !p.at(0).in_branch && p.at(0).t0_ms == -1.0);

  const ProfileLog::Summary s = p.summary();
  CHECK(s.n == 3 && s.mean_ms == (0.5 + 0.25 + 1.5) / 3 && s.flops_per_launch == (6e9 + 2e9 + 1e9) / 3 &&
        s.bytes_per_launch == (3e6 + 1e6 + 5e6) / 3);
  ProfileLog none = three_records(Pass::none);
  none.have_ms = true;
  CHECK(throws(DAC_E_STATE, "nothing profiled", [&] { none.summary(); }));
  ProfileLog empty;
  empty.enable(ProfileLog::ALL);
  empty.begin_pass(Pass::events);
  empty.have_ms = true;
  CHECK(throws(DAC_E_STATE, "nothing profiled", [&] { empty.summary(); }));
  p.enable(-1);                                                                  // disabling clears the records
  CHECK(p.rec.empty() && p.pass == Pass::none && throws(DAC_E_STATE, "nothing profiled", [&] { p.summary(); }));

  // c312 a: 2 launches, 2.00 ms, 7e9 flops -> 1000.0 us each, 3.5 TF/s; c350 b: 1 x 250.0 us, 8.0 TF/s.
  ProfileLog r = three_records(Pass::events);
  r.rec[0].ms = 0.5; r.rec[1].ms = 0.25; r.rec[2].ms = 1.5;
  char* buf = nullptr;
  size_t len = 0;
  FILE* f = open_memstream(&buf, &len);
  r.report(f);
  fclose(f);
  const char* want = "[dac conv profile] 3 launches, 2.25 ms total\n"
                     "       2 x   1000.0 us =     2.00 ms      3.5 TF/s  c312 a\n"
                     "       1 x    250.0 us =     0.25 ms      8.0 TF/s  c350 b\n";
  CHECK(std::string(buf, len) == want);
  if (std::string(buf, len) != want) printf("report was:\n%s", buf);
  free(buf);
}

static void check_pass_state() {
  ProfileLog p;
  p.enable(312);
  CHECK(p.on() && p.wants(312) && !p.wants(350) && p.pass == Pass::none);
  p.stamps = true;
  p.begin_pass(Pass::counting);
  p.counted = 2;
  CHECK(throws(DAC_E_STATE, "differ", [&] { p.check_complete(); }));
  p.begin_pass(Pass::stamps);
  p.stamps = false;                                                              // the next pass will be eager
  CHECK(p.pass == Pass::stamps);
  p.enable(ProfileLog::ALL);
  CHECK(p.wants(312) && p.wants(350));
  p.enable(-1);
  CHECK(!p.on() && !p.wants(312));
}

static void check_symbols() {
  const char* conv[] = {"conv_kernel", "conv2_kernel", "conv3_kernel", "conv3i_kernel", "conv3w_kernel",
                        "conv_down_kernel", "conv7_kernel", "conv3n_kernel", "conv8_kernel", "conv3q_kernel",
                        "conv3r_kernel", "conv_part_reduce_kernel"};
  for (const char* k : conv) {
    const std::string n(k), mangled = "_ZN3dac" + std::to_string(n.size()) + n;
    CHECK(symbol_args(n) == KernArgs::conv);
    CHECK(symbol_args(n + "<__half, 128, 128, 4, 2>") == KernArgs::conv);
    CHECK(symbol_args("void dac::" + n + "<float, 3, 3>(dac::ConvArgs, int)") == KernArgs::conv);
    CHECK(symbol_args(mangled + "IDF16_Li128ELi128ELi4ELi2ELi128ELb1EEEvNS_8ConvArgsEi") == KernArgs::conv);
  }
  CHECK(symbol_args("rbfuse_kernel") == KernArgs::rb && symbol_args("rbfuse_kernel<__half, 128>") == KernArgs::rb);
  CHECK(symbol_args("_ZN3dac13rbfuse_kernelIDF16_Li128EEEvNS_6RbArgsEi") == KernArgs::rb);
  CHECK(symbol_args("_ZN3dac23conv_part_reduce_kernelIDF16_EEvNS_8ConvArgsEim") == KernArgs::conv);
  for (const char* k : {"convert_rows_kernel", "myconv_kernel2", "", "conv_kernel2", "xconv_kernel", "_ZN3dac",
                        "_ZN3dac19convert_rows_kernelIfEEvPfi", "_ZN3dac14myconv_kernel2EPv", "_ZN3dac99conv_kernel",
                        "_ZN3dac99999999999999999999999conv_kernel", "stamp_init_kernel", "conv_kernel_helper<conv_kernel>"})
    CHECK(symbol_args(k) == KernArgs::none);
}

int main() {
  check_reduce();
  check_at_summary_report();
  check_pass_state();
  check_symbols();
  if (failures) {
    printf("%d check(s) failed\n", failures);
    return 1;
  }
  printf("profiler_check: all checks passed\n");
  return 0;
}

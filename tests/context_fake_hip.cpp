// context_fake_hip.cpp -- the lifetime of everything a context reserves, on the CPU (tests/test_context_lifetime_cpu.py).
//
// csrc/adsb_context.cpp, adsb_ring.cpp, adsb_decim.cpp and adsb_replay_host.cpp are compiled AS THEY ARE by
// g++ under AddressSanitizer + UBSan and linked against this file, which is three things:
//   * a counting fake of the HIP runtime: it keeps the live set of device allocations, pinned allocations, events and
//     streams, aborts on a free / destroy of anything that is not live (a double free, a derived pointer), fills fresh
//     memory with a poison byte, and can be armed so that the n-th runtime call from now fails with hipErrorOutOfMemory
//     (calls that release or only describe an error are not counted and never fail: their results are ignored by design);
//   * stubs, all succeeding, of what those units call below them (launch_*, scan_resident_blocks, submit ...);
//   * the driver: the assertions listed at main().
// No GPU, no decoding.
#include <map>

#include "../dump1090_rs_amd/csrc/adsb_ctx.h"

using namespace adsb::host;

// ---------------------------------------------------------------------------------------------------------------------
// the fake runtime
namespace {

enum LiveKind { kLiveDevice, kLivePinned, kLiveEvent, kLiveStream, kLiveRegistered };
const char *kind_name[] = {"device memory", "pinned memory", "event", "stream", "registered host range"};
std::map<void *, LiveKind> &g_live = *new std::map<void *, LiveKind>;   // (outlives main: the pool's streams stay reachable)
uint64_t g_calls = 0;        // fallible runtime calls so far
uint64_t g_fail_at = 0;      // the call with this number fails (0: none)
bool g_fired = false;
constexpr unsigned char kPoison = 0xA5;

[[noreturn]] void die(const char *what, const void *p)
{
    std::fprintf(stderr, "fake HIP: %s %p\n", what, p);
    std::abort();
}

// every fallible call starts with this
bool fails()
{
    if (++g_calls != g_fail_at) return false;
    g_fired = true;
    return true;
}
#define FALLIBLE() \
    if (fails()) return hipErrorOutOfMemory

hipError_t make(void **out, size_t bytes, LiveKind kind)
{
    void *p = std::malloc(bytes ? bytes : 1);
    if (!p) return hipErrorOutOfMemory;
    std::memset(p, kPoison, bytes ? bytes : 1);
    g_live[p] = kind;
    *out = p;
    return hipSuccess;
}

hipError_t unmake(void *p, LiveKind kind, const char *call)
{
    if (!p) return hipSuccess;   // (as the runtime: freeing null is a no-op)
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second != kind) die(call, p);
    g_live.erase(it);
    std::free(p);
    return hipSuccess;
}

void arm(uint64_t nth)
{
    g_fail_at = g_calls + nth;
    g_fired = false;
}
bool disarm()
{
    g_fail_at = 0;
    return g_fired;
}

// the live set without the streams (the pool's stay for the life of the process)
std::map<void *, LiveKind> live_without_streams()
{
    std::map<void *, LiveKind> m;
    for (const auto &e : g_live)
        if (e.second != kLiveStream) m.insert(e);
    return m;
}

}  // namespace

extern "C" {
hipError_t hipGetDeviceCount(int *n) { FALLIBLE(); *n = 1; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t *prop, int)
{
    FALLIBLE();
    std::memset(prop, 0, sizeof *prop);
    std::strcpy(prop->gcnArchName, "gfx950:sramecc+:xnack-");
    prop->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipSetDevice(int) { FALLIBLE(); return hipSuccess; }
hipError_t hipGetDevice(int *d) { FALLIBLE(); *d = 0; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "fake HIP error"; }
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) { FALLIBLE(); *least = 0, *greatest = -2; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { FALLIBLE(); return make((void **)s, 1, kLiveStream); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { FALLIBLE(); return make((void **)s, 1, kLiveStream); }
hipError_t hipExtStreamCreateWithCUMask(hipStream_t *s, uint32_t, const uint32_t *) { FALLIBLE(); return make((void **)s, 1, kLiveStream); }
hipError_t hipStreamDestroy(hipStream_t s) { return unmake(s, kLiveStream, "hipStreamDestroy of a stream that is not live"); }
hipError_t hipStreamSynchronize(hipStream_t s)
{
    if (s && g_live.find(s) == g_live.end()) die("hipStreamSynchronize on a stream that is not live", s);
    FALLIBLE();
    return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t n) { FALLIBLE(); return make(p, n, kLiveDevice); }
hipError_t hipFree(void *p) { return unmake(p, kLiveDevice, "hipFree of what is not a live device allocation"); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { FALLIBLE(); return make(p, n, kLivePinned); }
hipError_t hipHostFree(void *p) { return unmake(p, kLivePinned, "hipHostFree of what is not a live pinned allocation"); }
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned)
{
    if (g_live.find(host) == g_live.end()) die("hipHostGetDevicePointer of what is not live", host);
    FALLIBLE();
    *dev = host;
    return hipSuccess;
}
hipError_t hipHostRegister(void *p, size_t, unsigned) { FALLIBLE(); g_live[p] = kLiveRegistered; return hipSuccess; }
hipError_t hipHostUnregister(void *p)
{
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second != kLiveRegistered) die("hipHostUnregister of what is not registered", p);
    g_live.erase(it);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { FALLIBLE(); return make((void **)e, 1, kLiveEvent); }
hipError_t hipEventDestroy(hipEvent_t e) { return unmake(e, kLiveEvent, "hipEventDestroy of an event that is not live"); }
hipError_t hipMemset(void *dst, int v, size_t n) { FALLIBLE(); std::memset(dst, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t) { FALLIBLE(); std::memset(dst, v, n); return hipSuccess; }
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) { FALLIBLE(); std::memcpy(dst, src, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t) { FALLIBLE(); std::memcpy(dst, src, n); return hipSuccess; }
}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// what the units under test call below them: it succeeds
namespace adsb {
int scan_resident_blocks() { return 16; }   // (a small grid: short AP lists, the test's contexts stay a few MB)
int launch_reset(Counters *ctr, uint32_t *bitmap, uint32_t bitmap_lg, void *)
{
    std::memset(ctr, 0, sizeof(Counters));
    std::memset(bitmap, 0, bitmap_alloc_words(bitmap_lg) * sizeof(uint32_t));
    return 0;
}
int launch_rx_set_fill(const unsigned long long *, uint32_t, unsigned long long *, uint32_t, uint32_t, uint32_t *, void *) { return 0; }
int launch_rx_set_lookup(const unsigned long long *, uint32_t, const unsigned long long *, uint32_t, uint32_t, uint32_t *, void *) { return 0; }
int launch_decim(const DecimParams &, void *) { return 0; }
uint32_t decim_row_len(uint32_t, uint32_t n_taps) { return n_taps; }
namespace host {
void soapy_u8_table(int16_t *out256) { for (int x = 0; x < 256; x++) out256[x] = (int16_t)((x - 127) * 256); }
bool one_launch_pass(const adsb_ctx *, uint32_t) { return false; }
hipStream_t next_scan_stream(const adsb_ctx *c, uint32_t) { return c->scan_stream[0]; }
int submit(adsb_ctx *, const void *, SrcFormat, uint64_t, bool, hipEvent_t) { return ADSB_OK; }
int demod_device(adsb_ctx *, const void *, uint64_t, std::vector<adsb_msg> &, SrcFormat) { return ADSB_OK; }
void append_piece(const adsb_ctx *, std::vector<adsb_msg> &, uint64_t, std::vector<adsb_msg> &, adsb_stats &, std::vector<adsb_signal_stats> &) {}
int deliver(adsb_ctx *, std::vector<adsb_msg> &, adsb_msg *, size_t, size_t *n_out)
{
    if (n_out) *n_out = 0;
    return ADSB_OK;
}
}  // namespace host
}  // namespace adsb

// ---------------------------------------------------------------------------------------------------------------------
// the driver
namespace {

int g_checks = 0;
#define REQUIRE(cond, ...)                                             \
    do {                                                               \
        g_checks++;                                                    \
        if (!(cond)) {                                                 \
            std::fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                         \
            std::fprintf(stderr, "\n");                                \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

void require_same_live(const std::map<void *, LiveKind> &before, const char *what, uint64_t n)
{
    const auto now = live_without_streams();
    for (const auto &e : now)
        REQUIRE(before.count(e.first), "%s, call %llu failing: a live %s was left behind", what, (unsigned long long)n, kind_name[e.second]);
    for (const auto &e : before)
        REQUIRE(now.count(e.first), "%s, call %llu failing: a %s that was live before is gone", what, (unsigned long long)n, kind_name[e.second]);
}

adsb_ctx *create(size_t max_chunks)
{
    adsb_ctx *c = nullptr;
    const int rc = adsb_create(&c, 0, max_chunks);
    REQUIRE(rc == ADSB_OK && c, "adsb_create(%zu) = %d", max_chunks, rc);
    return c;
}

bool scores_on_device(const adsb_ctx *c) { return c->score.si != nullptr; }

bool rx_wired(const adsb_ctx *c)
{
    bool ok = c->rx_set[0] && c->rx_set[1] && c->d_rx_failed;
    for (int si = 0; si < c->n_slots; si++) {
        const Slot &sl = c->slot[si];
        ok = ok && sl.rx.rx_map && sl.rx.first && sl.rx.rx_slot && sl.rx.out_add_rx && sl.h_rx_map && sl.h_add_rx;
    }
    return ok;
}
bool sig_wired(const adsb_ctx *c)
{
    bool ok = true;
    for (int si = 0; si < c->n_slots; si++) {
        const Slot &sl = c->slot[si];
        ok = ok && sl.h_sig && sl.h_sig_dev && sl.d_sig_part && sl.d_sig_ticket;
    }
    return ok;
}
bool shard_wired(const adsb_ctx *c, int k, bool fresh)
{
    const auto &j = c->shard[k];
    return j.h_addrs && j.h_addrs_dev && (!fresh || (j.h_fresh && j.h_fresh_dev && j.d_fresh_seen && j.h_earlier && j.h_earlier_dev));
}
bool ring_wired(const adsb_ctx *c)
{
    bool ok = c->ring_samples != 0;
    for (int k = 0; k < c->n_slots; k++) ok = ok && c->ring[k].h_iq && c->ring[k].h_iq_dev && c->ring[k].d_iq;
    return ok;
}

adsb_decim *make_decim(adsb_ctx *c)
{
    const int16_t taps[3] = {8192, 16384, 8192};
    adsb_decim *d = nullptr;
    const int rc = adsb_decim_create(c, 2, taps, 3, 15, &d);
    REQUIRE(rc == ADSB_OK && d, "adsb_decim_create = %d", rc);
    return d;
}

// 1. everything that can be reserved, then adsb_destroy: nothing but streams stays live
void everything_reserved(size_t max_chunks, bool ring_u8)
{
    const auto before = live_without_streams();
    adsb_ctx *c = create(max_chunks);
    REQUIRE(adsb_set_signal_stats(c, 1) == ADSB_OK && sig_wired(c), "signal statistics");
    REQUIRE(adsb_set_receivers(c, 1) == ADSB_OK, "one receiver");
    REQUIRE(adsb_set_receiver_scoring(c, 1) == ADSB_OK, "receiver scoring");
    const void *set_of_one = c->rx_set[0];
    REQUIRE(adsb_set_receivers(c, 2) == ADSB_OK, "two receivers");
    if (scores_on_device(c)) {
        REQUIRE(rx_wired(c), "receiver scoring: a slot's views");
        REQUIRE(c->rx_set_alloc_lg == rx_set_lg_for(2) && rx_set_lg_for(2) != rx_set_lg_for(1) && set_of_one, "the keyed sets were re-made");
    } else {
        REQUIRE(!c->h_rx_block && !c->rx_set[0], "a context that never scores on the device reserves nothing for receiver scoring");
    }
    REQUIRE((ring_u8 ? adsb_ring_create_u8(c, kChunkSamples) : adsb_ring_create(c, kChunkSamples)) == ADSB_OK && ring_wired(c), "ring");
    REQUIRE(ensure_fallback(c) == ADSB_OK && c->fb.d_hits && c->fb.d_dap && c->fb.h_rec && c->fb.h_rec_dev, "fallback lists");
    for (size_t bytes : {1000u, 5000u, 3000u, 70000u}) {
        REQUIRE(ensure_stage(c, bytes) == ADSB_OK && c->d_stage && c->stage_bytes >= bytes, "ensure_stage(%zu)", bytes);
        REQUIRE(ensure_host_stage(c, bytes) == ADSB_OK && c->h_stage && c->h_stage_dev && c->h_stage_bytes >= bytes, "ensure_host_stage(%zu)", bytes);
        std::memset(c->d_stage, 1, bytes);   // (ASan: the buffer is as large as it says)
        std::memset(c->h_stage, 1, bytes);
    }
    REQUIRE(ensure_addrs(c, 10, IcaoFilter::kSize) == ADSB_OK && ensure_addrs(c, 5000, 8192) == ADSB_OK && c->addrs_cap == 8192, "ensure_addrs");
    REQUIRE(ensure_rx_keys(c, 10) == ADSB_OK && ensure_rx_keys(c, 20000) == ADSB_OK && c->rx_keys_cap >= 20000, "ensure_rx_keys");
    REQUIRE(ensure_widen(c) == ADSB_OK && ensure_widen(c) == ADSB_OK && c->d_widen, "the CU8 widen buffer");
    REQUIRE(ensure_shard_lists(c, 0, false) == ADSB_OK && shard_wired(c, 0, false) && !c->shard[0].h_fresh, "shard lists without fresh_list");
    REQUIRE(ensure_shard_lists(c, 1, true) == ADSB_OK && shard_wired(c, 1, true), "shard lists with fresh_list");
    REQUIRE(ensure_shard_lists(c, 0, true) == ADSB_OK && shard_wired(c, 0, true), "shard lists, fresh_list added later");
    int dummy = 0;
    REQUIRE(adsb_host_register(c, &dummy, sizeof dummy) == ADSB_OK, "adsb_host_register");
    adsb_decim *d = make_decim(c);
    std::vector<int16_t> iq(2 * 5000, 0);
    size_t n_out = 0;
    REQUIRE(adsb_decim_demod_iq(d, ADSB_DECIM_CS16, iq.data(), 1000, nullptr, 0, &n_out) == ADSB_OK, "decimator, 1000 samples");
    REQUIRE(adsb_decim_demod_iq(d, ADSB_DECIM_CS16, iq.data(), 5000, nullptr, 0, &n_out) == ADSB_OK, "decimator, 5000 samples: the staging grows");
    adsb_decim_destroy(d);
    adsb_destroy(c);
    require_same_live(before, "everything reserved, then adsb_destroy", 0);
}

// 4. created, used for nothing, destroyed
void unused_context(size_t max_chunks)
{
    const auto before = live_without_streams();
    adsb_destroy(create(max_chunks));
    require_same_live(before, "an unused context", 0);
}

// 2. every n-th runtime call of adsb_create failing; an unarmed adsb_create follows every failure
uint64_t create_failures(size_t max_chunks)
{
    for (uint64_t n = 1;; n++) {
        const auto before = live_without_streams();
        adsb_ctx *c = reinterpret_cast<adsb_ctx *>(&n);
        arm(n);
        const int rc = adsb_create(&c, 0, max_chunks);
        if (!disarm()) {   // the call was through before its n-th runtime call: n - 1 is what a successful one makes
            REQUIRE(rc == ADSB_OK && c, "adsb_create(%zu) unarmed = %d", max_chunks, rc);
            adsb_destroy(c);
            REQUIRE(n > 50, "adsb_create made only %llu runtime calls", (unsigned long long)n - 1);
            return n - 1;
        }
        REQUIRE(rc != ADSB_OK && c == nullptr, "adsb_create(%zu) with call %llu failing = %d, *out = %p", max_chunks, (unsigned long long)n, rc, (void *)c);
        require_same_live(before, "adsb_create", n);
        unused_context(max_chunks);
    }
}

// 3. every n-th runtime call of one lazy reservation failing, in a context that `prepare` has brought to where the
// reservation is due: an error and the live set as before.  The retry is the next attempt, which has to get past the call
// that failed before -- so the attempt that finally succeeds follows a failure at every one of its calls -- and after it
// every view of the feature must be wired.
template <class Prepare, class Call, class Wired>
uint64_t lazy_failures(const char *what, size_t max_chunks, Prepare prepare, Call call, Wired wired)
{
    adsb_ctx *c = create(max_chunks);
    prepare(c);
    for (uint64_t n = 1;; n++) {
        const auto before = live_without_streams();
        arm(n);
        const int rc = call(c);
        if (!disarm()) {
            REQUIRE(rc == ADSB_OK, "%s after %llu failures = %d (%s)", what, (unsigned long long)n - 1, rc, adsb_last_error(c));
            REQUIRE(wired(c), "%s: after %llu failures and a call that succeeded not every view is wired", what, (unsigned long long)n - 1);
            adsb_destroy(c);
            REQUIRE(n > 1, "%s made no runtime call", what);
            return n - 1;
        }
        REQUIRE(rc != ADSB_OK, "%s with call %llu failing returned ADSB_OK", what, (unsigned long long)n);
        require_same_live(before, what, n);
    }
}

// ... and of a grower that replaces a buffer it holds: the old one goes first (nothing reads it, and the two never add up),
// so a failure leaves the buffer absent and its size zero -- nothing else -- and the retry succeeds
template <class Call, class Absent>
void grower_failure(const char *what, Call call, Absent absent)
{
    adsb_ctx *c = create(1);
    REQUIRE(call(c, 1000) == ADSB_OK, "%s(1000)", what);
    const size_t live_before = live_without_streams().size();
    arm(1);
    const int rc = call(c, 100000);
    REQUIRE(disarm() && rc != ADSB_OK && absent(c), "%s(100000) with its reservation failing = %d", what, rc);
    REQUIRE(live_without_streams().size() == live_before - 1, "%s: a failed growth left something behind", what);
    REQUIRE(call(c, 100000) == ADSB_OK && !absent(c), "%s(100000), retried", what);
    adsb_destroy(c);
}

}  // namespace

// What is asserted (the numbers as in the test's docstring):
//   1. with everything reserved that can be -- in a small and in a large context, with a CS16 and with a CU8 ring -- after
//      adsb_destroy only streams are live;
//   2. adsb_create with its n-th runtime call failing, for every n: an error, *out null, the live set as before, and an
//      unarmed adsb_create succeeds;
//   3. every lazy reservation with its n-th runtime call failing, for every n: an error, the live set as before, an
//      unarmed retry succeeds and every view of the feature is wired;
//   4. a context created and destroyed releases exactly what it reserved.
int main()
{
    const size_t kSmall = 1, kLarge = 17;   // 17: the smallest context that scores on the device
    {
        DeviceGuard counts_the_devices_once_per_process(0);
    }
    const auto at_start = live_without_streams();
    REQUIRE(at_start.empty(), "%zu reservations live before anything was created", at_start.size());

    // 2 (the first failures fall into the making of the device's stream pool, which the retry then completes)
    const uint64_t n_large = create_failures(kLarge);
    unused_context(kSmall);   // (a small context's pool streams: a refused CU mask is tolerated by design, so none of adsb_create's failures)
    const uint64_t n_small = create_failures(kSmall);
    // 4 and 1
    for (size_t mc : {kSmall, kLarge}) {
        unused_context(mc);
        everything_reserved(mc, false);
        everything_reserved(mc, true);
    }
    {
        adsb_ctx *c = create(kLarge);
        REQUIRE(scores_on_device(c), "a context of %zu buffers scores on the device", kLarge);
        adsb_destroy(c);
        c = create(kLarge - 1);
        REQUIRE(!scores_on_device(c), "a context of %zu buffers does not", kLarge - 1);
        adsb_destroy(c);
    }
    // 3
    uint64_t n_lazy = 0;
    auto nothing = [](adsb_ctx *) {};
    for (size_t mc : {kSmall, kLarge}) {
        n_lazy += lazy_failures("ensure_signal_stats", mc, nothing, [](adsb_ctx *c) { return adsb_set_signal_stats(c, 1); }, sig_wired);
        n_lazy += lazy_failures("ensure_fallback", mc, nothing, ensure_fallback,
                                [](adsb_ctx *c) { return c->fb.d_hits && c->fb.d_dap && c->fb.h_rec && c->fb.h_rec_dev; });
        n_lazy += lazy_failures("ensure_shard_lists(fresh)", mc, nothing, [](adsb_ctx *c) { return ensure_shard_lists(c, 0, true); },
                                [](adsb_ctx *c) { return shard_wired(c, 0, true); });
        n_lazy += lazy_failures("ensure_shard_lists(fresh, after plain)", mc, [](adsb_ctx *c) { (void)ensure_shard_lists(c, 0, false); },
                                [](adsb_ctx *c) { return ensure_shard_lists(c, 0, true); }, [](adsb_ctx *c) { return shard_wired(c, 0, true); });
        n_lazy += lazy_failures("adsb_ring_create", mc, nothing, [](adsb_ctx *c) { return adsb_ring_create(c, kChunkSamples); }, ring_wired);
        n_lazy += lazy_failures("adsb_ring_create_u8", mc, nothing, [](adsb_ctx *c) { return adsb_ring_create_u8(c, kChunkSamples); }, ring_wired);
    }
    n_lazy += lazy_failures("ensure_rx_scoring", kLarge, [](adsb_ctx *c) { (void)adsb_set_receivers(c, 2); },
                            [](adsb_ctx *c) { return adsb_set_receiver_scoring(c, 1); }, rx_wired);
    {
        // adsb_decim_create: the handle's own registry
        adsb_ctx *c = create(kSmall);
        const int16_t taps[3] = {8192, 16384, 8192};
        for (uint64_t n = 1;; n++) {
            const auto before = live_without_streams();
            adsb_decim *d = nullptr;
            arm(n);
            const int rc = adsb_decim_create(c, 2, taps, 3, 15, &d);
            if (!disarm()) {
                REQUIRE(rc == ADSB_OK && d && n > 3, "adsb_decim_create unarmed = %d", rc);
                adsb_decim_destroy(d);
                n_lazy += n - 1;
                break;
            }
            REQUIRE(rc != ADSB_OK && !d, "adsb_decim_create with call %llu failing = %d", (unsigned long long)n, rc);
            require_same_live(before, "adsb_decim_create", n);
        }
        adsb_destroy(c);
    }
    grower_failure("ensure_stage", ensure_stage, [](adsb_ctx *c) { return !c->d_stage && !c->stage_bytes; });
    grower_failure("ensure_host_stage", ensure_host_stage, [](adsb_ctx *c) { return !c->h_stage && !c->h_stage_dev && !c->h_stage_bytes; });
    grower_failure("ensure_addrs", [](adsb_ctx *c, size_t n) { return ensure_addrs(c, n, n); }, [](adsb_ctx *c) { return !c->d_addrs && !c->addrs_cap; });
    grower_failure("ensure_rx_keys", ensure_rx_keys, [](adsb_ctx *c) { return !c->d_rx_keys && !c->rx_keys_cap; });
    {
        // the keyed sets re-made for another number of receivers: a failure leaves none (and the slots' buffers as they
        // were), the retry makes both
        adsb_ctx *c = create(kLarge);
        REQUIRE(adsb_set_receivers(c, 1) == ADSB_OK && adsb_set_receiver_scoring(c, 1) == ADSB_OK && rx_wired(c), "receiver scoring, one receiver");
        for (uint64_t n = 1; n <= 2; n++) {
            const size_t live_before = live_without_streams().size();
            const bool had = c->rx_set[0] != nullptr;
            arm(n);
            const int rc = adsb_set_receivers(c, 2);
            REQUIRE(disarm() && rc != ADSB_OK && !c->rx_set[0] && !c->rx_set[1] && !c->rx_set_alloc_lg, "re-making the keyed sets, call %llu failing", (unsigned long long)n);
            REQUIRE(live_without_streams().size() == live_before - (had ? 2 : 0), "re-making the keyed sets: a failure left something behind");
            REQUIRE(adsb_get_receivers(c) == 2, "the number of receivers is set whatever comes of the sets");
            REQUIRE(adsb_set_receivers(c, 1) == ADSB_OK && rx_wired(c), "retry with one receiver");
        }
        adsb_destroy(c);
    }
    require_same_live(at_start, "the whole run", 0);
    std::printf("context lifetime ok: %d checks; runtime calls of adsb_create: %llu large, %llu small; "
                "%llu lazy-reservation failures injected; live at exit: %zu streams\n",
                g_checks, (unsigned long long)n_large, (unsigned long long)n_small, (unsigned long long)n_lazy,
                g_live.size());
    return 0;
}

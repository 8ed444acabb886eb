// adsb_feed -- the receive loop of dump1090_rs/src/main.rs:154-201 with the SDR replaced by a
// file or a pipe and the demodulation done by libadsb_hip: read 2.4 MSPS i16 IQ, demodulate,
// print every frame as "*<hex>;" and send "*<hex>;\n" to raw-TCP clients (port 30002 in the
// reference, main.rs:46) so that downstream tools (adsb_deku's radar, anything that speaks
// the dump1090 raw format) can consume it.
//
//   adsb_feed [--device N] [--port P] [--quiet] [--mem-order] [--format cs16|cu8|cf32|s16real] [--fix none|1bit|2bit] [--buffers K]
//             [--latency-ms T] [--readers R] [--stats [SECONDS]] [--decimate D | --resample L/M] [--shift HZ] [--scale G]
//             [--input-stats [SECONDS]] <capture.iq | ->
//
// --decimate D (2..16): the input is sampled at D x 2.4 MS/s, in the format --format names, and goes through the
// library's decimator with its default taps (adsb_decim_default_taps) in front of the demodulation: the output lines are
// those of the decimated stream, cut into 131072-sample buffers as that stream would be.  This path is the blocking call
// (adsb_decim_demod_iq), K buffers of output per call, not the ring: --latency-ms and --readers do not apply to it.
//
// --resample L/M: the input is sampled at 2.4 MS/s x M / L (an Airspy at 10 MS/s: 6/25; include/adsb_hip.h, "Resampling")
// and goes through the library's resampler with its default taps (adsb_resamp_default_taps) the same way, through
// adsb_resamp_demod_iq.  A call takes the input of K output buffers, K rounded up to a multiple of L's odd part so that
// the input of a call is a whole number of samples and every call ends on a buffer boundary of the resampled stream.
// Not together with --decimate.
//
// --shift HZ (signed; only with --decimate or --resample): the radio was offset-tuned, and the spectrum is moved by HZ on
// its way into the filter (include/adsb_hip.h, "Frequency shift": adsb_mix_for_shift, adsb_mix_table, adsb_mix_set_*).  A
// radio tuned 2.4 MHz below 1090 MHz: --shift -2400000.  A shift whose table would be longer than 256 is a usage error.
//
// --format cf32 | s16real (only with --decimate or --resample; include/adsb_hip.h, "Sample formats"): cf32 is complex
// float32, re then im, 8 bytes per sample -- what SoapySDR applications, GNU Radio file sinks, gqrx and `airspy_rx -t 0`
// write -- converted on the device as clamp(rint(x G)); --scale G (only with --format cf32; finite, 0 < G <= 2^31) sets G,
// 32768 by default.  s16real is one real int16 per sample, what `airspy_rx -t 3` writes; its band sits at a quarter of the
// sample rate, and --shift brings it down with the exact quarter-turn table:
//   Airspy R2 raw, 20 MS/s:    adsb_feed --format s16real --resample 3/25 --shift -5000000
//   Airspy Mini raw, 12 MS/s:  adsb_feed --format s16real --decimate 5 --shift -3000000
// cf32 that is already at 2.4 MS/s: --format cf32 --resample 1/1 (the default taps of 1/1 are a plain delay of four
// samples).  --mem-order means nothing to either format.
//
// --stats turns the signal statistics on (adsb_set_signal_stats) and prints what a receiver's gain is tuned by to
// STDERR, every SECONDS (default 1) over the buffers since the last line and once more, as the last line, over the
// whole input: the number of buffers, the noise floor (the median magnitude), the mean power and the peak in dBFS, and
// the shares of clipped and of strong (above -3 dBFS) samples.  stdout and the TCP stream are byte for byte what they
// are without the flag.
//
// --input-stats (only with --decimate or --resample) turns the input statistics of the decimator or resampler on
// (include/adsb_hip.h, "Input statistics": adsb_instat_set_*): the RAW input, at the radio's own rate and in its own
// format, counted on the device in front of the filter -- the rail hits, the DC offset and the NaNs that --stats, which
// looks at the filtered 2.4 MS/s stream, can no longer see.  Lines beginning "adsb_feed: input stats (" go to STDERR, every
// SECONDS (default 1) over the input since the last line and once more, as the last line, over the whole input: samples,
// mean power and peak in dBFS, the DC offset in LSB, the shares of clipped and of NaN samples, the I/Q gain balance in dB
// and the bits in use.  stdout, the TCP stream and the lines of --stats are byte for byte what they are without the flag.
//   Airspy R2 raw, 20 MS/s, gain set by the ADC's own rail hits:
//                              adsb_feed --format s16real --resample 3/25 --shift -5000000 --input-stats
//
// --fix 1bit repairs DF17/18 frames with one flipped bit from aircraft already heard, --fix 2bit with one or two
// (adsb_set_error_correction);
// none, the default, is the reference's output.
//
// Input is the reference's capture format (src/utils.rs:8-20, save_test_data): little-endian
// i16 pairs, im first; --mem-order takes {re, im} pairs instead.  --format cu8 takes what rtl_sdr writes
// (a file or a pipe): unsigned bytes, I then Q, 2 per sample, widened on the device through T_soapy
// (include/adsb_hip.h, "8-bit IQ"); cs16, the default, is the i16 input above.  The stream is cut into
// 131072-sample buffers exactly as consecutive SDR reads would be (no carry-over between
// buffers, src/lib.rs:36-44); up to K of them (default 64) travel to the GPU per pass through the
// pinned ring (adsb_ring_*), so reading, the copy and the scan overlap.  A slot does not wait to
// fill up: T ms (default 100) after its first whole buffer was complete, the whole buffers read so
// far are submitted as a shorter pass -- a deadline, not an idle timer: a live 2.4 MSPS pipe delivers
// data all the time, a buffer every 55 ms, and would otherwise sit 3.5 s in a 64-buffer slot -- and
// the begun buffer moves on to the next slot, so the cuts stay where consecutive reads of 131072
// samples put them.  Raw-TCP clients are written without blocking: one whose socket buffer stays
// full for T ms (it stopped reading) is dropped, as the reference drops a client whose write fails
// (main.rs:184-200); one that is merely slower than a burst of output is waited for that long, so an
// offline replay, which produces lines far faster than real time, loses nobody who reads.  New
// clients are accepted while waiting for input too.  A pass with more frames than the output array gets them all
// (adsb_fetch_messages).  The ICAO filter is never flushed, as in the reference's loop.
// A regular file cannot trickle, so its slots are filled by R threads (default 4) that each pread() and
// swap their own part of the slot: one thread in read() copies out of the page cache at 6-10 GB/s, a
// fifth of what the ring takes.  Pipes and sockets are read by the one loop below.
// No GPU -> exits non-zero.
#include <arpa/inet.h>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <netinet/in.h>
#include <poll.h>
#include <condition_variable>
#include <mutex>
#include <string>
#include <sys/socket.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../../include/adsb_hip.h"

namespace {

struct Clients {
    int listener = -1;
    std::vector<int> socks;
    unsigned long long dropped = 0;

    bool listen_on(int port)
    {
        listener = ::socket(AF_INET, SOCK_STREAM, 0);
        if (listener < 0) return false;
        int one = 1;
        ::setsockopt(listener, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
        sockaddr_in a{};
        a.sin_family = AF_INET;
        a.sin_addr.s_addr = htonl(INADDR_ANY);  // main.rs:38: 0.0.0.0 by default
        a.sin_port = htons((uint16_t)port);
        if (::bind(listener, (sockaddr *)&a, sizeof(a)) != 0 || ::listen(listener, 16) != 0) return false;
        ::fcntl(listener, F_SETFL, ::fcntl(listener, F_GETFL, 0) | O_NONBLOCK);  // main.rs:150
        return true;
    }
    void accept_new()  // main.rs:155-158
    {
        if (listener < 0) return;
        for (;;) {
            const int s = ::accept(listener, nullptr, nullptr);
            if (s < 0) break;
            // never block on a client: a generous send buffer for bursts, then EAGAIN means it is not reading
            ::fcntl(s, F_SETFL, ::fcntl(s, F_GETFL, 0) | O_NONBLOCK);
            int sndbuf = 1 << 20;  // ~30 000 frames of backlog (the kernel may grant less)
            ::setsockopt(s, SOL_SOCKET, SO_SNDBUF, &sndbuf, sizeof(sndbuf));
            socks.push_back(s);
        }
    }
    // main.rs:184-199: drop a client when its write fails.  A full socket buffer (EAGAIN) is given
    // `budget_ms` to drain -- the client is reading, only slower than this burst -- and counts as a
    // failed write after that (a partly written line could not be completed later without queueing
    // per client).
    void send_all(const std::string &lines, int budget_ms)
    {
        for (size_t i = 0; i < socks.size();) {
            size_t off = 0;
            bool dead = false;
            const auto t0 = std::chrono::steady_clock::now();
            while (off < lines.size()) {
                const ssize_t w = ::send(socks[i], lines.data() + off, lines.size() - off, MSG_NOSIGNAL | MSG_DONTWAIT);
                if (w <= 0) {
                    if (w < 0 && errno == EINTR) continue;
                    if (w < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) {
                        const long spent = (long)std::chrono::duration_cast<std::chrono::milliseconds>(
                                               std::chrono::steady_clock::now() - t0).count();
                        pollfd p{socks[i], POLLOUT, 0};
                        if (spent < budget_ms && ::poll(&p, 1, (int)(budget_ms - spent)) > 0 && (p.revents & POLLOUT)) continue;
                    }
                    dead = true;
                    dropped++;
                    break;
                }
                off += (size_t)w;
            }
            if (dead) {
                ::close(socks[i]);
                socks.erase(socks.begin() + (long)i);
            } else {
                i++;
            }
        }
    }
    ~Clients()
    {
        for (int s : socks) ::close(s);
        if (listener >= 0) ::close(listener);
    }
};

// --stats: signal records folded together (sums; the peak is a maximum) -- adsb_signal_summary takes any number of
// records, so a run of any length is a handful of them: a new one is begun before a 32-bit count could wrap.
struct SignalFold {
    std::vector<adsb_signal_stats> folded;
    unsigned long long buffers = 0;
    void add(const adsb_signal_stats &r)
    {
        if (folded.empty() || (unsigned long long)folded.back().n_samples + r.n_samples > 0x7FFFFFFFull) folded.push_back(adsb_signal_stats{});
        adsb_signal_stats &f = folded.back();
        f.sum_power += r.sum_power, f.n_samples += r.n_samples, f.n_strong += r.n_strong, f.n_clipped += r.n_clipped;
        if (r.peak > f.peak) f.peak = r.peak;
        for (int b = 0; b < ADSB_SIGNAL_BINS; b++) f.hist[b] += r.hist[b];
        buffers++;
    }
    void clear() { folded.clear(), buffers = 0; }
    void print(const char *scope) const
    {
        adsb_signal_summary_t s{};
        if (adsb_signal_summary(folded.data(), folded.size(), &s) != ADSB_OK) return;
        std::fprintf(stderr, "adsb_feed: stats (%s): buffers %llu, floor %.3f dBFS, mean %.3f dBFS, peak %.3f dBFS, clipped %.6f %%, strong %.6f %%\n",
                     scope, buffers, s.median_dbfs, s.mean_power_dbfs, s.peak_dbfs, 100.0 * s.clipped_fraction, 100.0 * s.strong_fraction);
    }
};

// --input-stats: input records folded together.  The records' own sums are 64 bits wide, and adsb_input_summary takes
// any number of records: a new one is begun every 2^32 samples.
struct InputFold {
    std::vector<adsb_input_stats> folded;
    void add(const adsb_input_stats &r)
    {
        if (folded.empty() || folded.back().n_samples >> 32) folded.push_back(adsb_input_stats{});
        adsb_input_stats &f = folded.back();
        f.n_samples += r.n_samples, f.sum_re += r.sum_re, f.sum_im += r.sum_im, f.sum_re2 += r.sum_re2, f.sum_im2 += r.sum_im2;
        f.sum_re_im += r.sum_re_im, f.n_clipped += r.n_clipped, f.n_nan += r.n_nan;
        if (r.peak > f.peak) f.peak = r.peak;
        for (int b = 0; b < ADSB_INPUT_BINS; b++) f.hist[b] += r.hist[b];
    }
    void clear() { folded.clear(); }
    void print(const char *scope) const
    {
        adsb_input_summary_t s{};
        if (adsb_input_summary(folded.data(), folded.size(), &s) != ADSB_OK) return;
        std::fprintf(stderr, "adsb_feed: input stats (%s): samples %llu, mean %.3f dBFS, peak %.3f dBFS, dc re %.3f im %.3f LSB, clipped %.6f %%, nan %.6f %%, iq gain %.3f dB, bits %u\n",
                     scope, (unsigned long long)s.n_samples, s.mean_power_dbfs, s.peak_dbfs, s.dc_re, s.dc_im, 100.0 * s.clipped_fraction,
                     100.0 * s.nan_fraction, s.iq_gain_db, s.bits_used);
    }
};

int die(adsb_ctx *ctx, const char *what, int st)
{
    std::fprintf(stderr, "adsb_feed: %s: %s %s\n", what, adsb_strerror(st), ctx ? adsb_last_error(ctx) : "");
    if (ctx) adsb_destroy(ctx);
    return 1;
}

// Wait up to idle_ms for input (idle_ms < 0: for ever) and read once into dst[have, want).
// Returns the new fill; *eof at end of input, *idle when nothing arrived in time.
size_t read_once(int fd, char *dst, size_t have, size_t want, int idle_ms, bool *eof, bool *idle)
{
    *idle = false;
    for (;;) {
        pollfd p{fd, POLLIN, 0};
        const int pr = ::poll(&p, 1, idle_ms);
        if (pr == 0) {
            *idle = true;
            return have;
        }
        if (pr < 0) {
            if (errno == EINTR) continue;
            *eof = true;
            return have;
        }
        const ssize_t r = ::read(fd, dst + have, want - have);
        if (r < 0 && (errno == EINTR || errno == EAGAIN)) continue;
        if (r <= 0) {
            *eof = true;
            return have;
        }
        return have + (size_t)r;
    }
}

// file pairs are [im][re]: swap into the in-memory {re, im} (utils.rs:29-31).  A 16-bit rotate of each pair as
// one word: the compiler vectorises it; pair by pair the swap was the slowest stage of the feed.
void swap_pairs(char *bytes, size_t n_pairs)
{
    typedef uint32_t __attribute__((may_alias)) pair_word;
    pair_word *w = reinterpret_cast<pair_word *>(bytes);
    for (size_t k = 0; k < n_pairs; k++) w[k] = (w[k] << 16) | (w[k] >> 16);
}

// Fills slots from a regular file with `n` threads (the caller is one of them): every thread pread()s its
// own 4-byte-aligned part of [offset, offset + bytes) into its part of the slot and swaps it there.
class FileFill {
public:
    FileFill(int fd, int n, bool swap) : fd_(fd), swap_(swap)
    {
        for (int k = 1; k < n; k++) workers_.emplace_back([this, k] { run(k); });
    }
    ~FileFill()
    {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
            round_++;
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }
    // Reads up to `bytes` at `offset` into dst; returns what the file had (short only at its end).
    size_t fill(char *dst, off_t offset, size_t bytes)
    {
        const size_t parts = workers_.size() + 1;
        if (bytes < (size_t(1) << 20) || parts == 1) return part(dst, offset, bytes);
        {
            std::lock_guard<std::mutex> g(mu_);
            dst_ = dst, offset_ = offset, bytes_ = bytes;
            left_ = (int)workers_.size();
            got_.assign(parts, 0);
            round_++;
        }
        cv_.notify_all();
        const size_t mine = share(0, nullptr);
        got_[0] = part(dst, offset, mine);
        std::unique_lock<std::mutex> g(mu_);
        done_.wait(g, [this] { return left_ == 0; });
        size_t total = 0;   // the parts are contiguous: a short one ends the file
        for (size_t k = 0; k < parts; k++) {
            size_t want = 0;
            share(k, &want);
            total += got_[k];
            if (got_[k] < want) break;
        }
        return total;
    }

private:
    size_t share(size_t k, size_t *want) const   // part k = [k * per, min((k + 1) * per, bytes))
    {
        const size_t parts = workers_.size() + 1;
        const size_t per = ((bytes_ + parts - 1) / parts + 4095) & ~size_t(4095);
        const size_t lo = k * per < bytes_ ? k * per : bytes_;
        const size_t hi = lo + per < bytes_ ? lo + per : bytes_;
        if (want) *want = hi - lo;
        return k == 0 ? hi - lo : lo;
    }
    size_t part(char *dst, off_t offset, size_t bytes) const
    {
        size_t have = 0;
        while (have < bytes) {
            const ssize_t r = ::pread(fd_, dst + have, bytes - have, offset + (off_t)have);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) break;
            have += (size_t)r;
        }
        if (swap_) swap_pairs(dst, have / 4);   // (a capture ends on a whole pair or its last bytes are dropped below)
        return have;
    }
    void run(int k)
    {
        unsigned long long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> g(mu_);
            cv_.wait(g, [&] { return round_ != seen; });
            seen = round_;
            if (stop_) return;
            size_t want = 0;
            const size_t lo = share((size_t)k, &want);
            char *dst = dst_ + lo;
            const off_t at = offset_ + (off_t)lo;
            g.unlock();
            const size_t got = part(dst, at, want);
            g.lock();
            got_[(size_t)k] = got;
            if (--left_ == 0) done_.notify_one();
        }
    }
    int fd_;
    bool swap_;
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    unsigned long long round_ = 0;
    bool stop_ = false;
    char *dst_ = nullptr;
    off_t offset_ = 0;
    size_t bytes_ = 0;
    int left_ = 0;
    std::vector<size_t> got_;
};

}  // namespace

int main(int argc, char **argv)
{
    int device = 0, port = 0, buffers = 64, latency_ms = 100, out_cap = 0, readers = 4;
    bool quiet = false, mem_order = false, cu8 = false, stats = false;
    double stats_seconds = 1.0;
    bool input_stats = false;
    double input_stats_seconds = 1.0;
    int fix = ADSB_FIX_NONE, decimate = 0;
    unsigned res_up = 0, res_down = 0;
    bool shifted = false, scaled = false;
    long shift_hz = 0;
    float scale = 0;
    int in_format = ADSB_DECIM_CS16;   // (cu8 says ADSB_DECIM_8BIT: the ring path knows only that flag)
    uint32_t mix_k = 0, mix_period = 0;
    const char *path = nullptr;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
        else if (a == "--port" && i + 1 < argc) port = std::atoi(argv[++i]);
        else if (a == "--buffers" && i + 1 < argc) buffers = std::atoi(argv[++i]);
        else if (a == "--latency-ms" && i + 1 < argc) latency_ms = std::atoi(argv[++i]);
        else if (a == "--readers" && i + 1 < argc) readers = std::atoi(argv[++i]);
        else if (a == "--decimate" && i + 1 < argc) {
            decimate = std::atoi(argv[++i]);
            if (decimate < 2 || decimate > 16) path = nullptr, i = argc;
        }
        else if (a == "--resample" && i + 1 < argc) {
            char tail = 0;
            uint32_t n_taps = 0;
            if (std::sscanf(argv[++i], "%u/%u%c", &res_up, &res_down, &tail) != 2 ||
                adsb_resamp_default_taps(res_up, res_down, nullptr, 0, &n_taps, nullptr) != ADSB_ERR_CAPACITY)
                path = nullptr, i = argc;
        }
        else if (a == "--shift" && i + 1 < argc) {
            char *end = nullptr;
            shift_hz = std::strtol(argv[++i], &end, 10);
            shifted = true;
            if (end == argv[i] || *end != 0 || shift_hz < -2147483647L || shift_hz > 2147483647L) path = nullptr, i = argc;
        }
        else if (a == "--scale" && i + 1 < argc) {
            char *end = nullptr;
            scale = std::strtof(argv[++i], &end);
            scaled = true;
            if (end == argv[i] || *end != 0 || !(scale > 0.0f) || !(scale <= 2147483648.0f)) path = nullptr, i = argc;
        }
        else if (a == "--out-cap" && i + 1 < argc) out_cap = std::atoi(argv[++i]);  // frames the output array starts with (it grows)
        else if (a == "--stats") {
            stats = true;
            char *end = nullptr;   // SECONDS is optional: taken when the next argument is a positive number and nothing else
            const double v = i + 1 < argc ? std::strtod(argv[i + 1], &end) : 0.0;
            if (i + 1 < argc && end != argv[i + 1] && *end == 0 && v > 0) stats_seconds = v, i++;
        }
        else if (a == "--input-stats") {
            input_stats = true;
            char *end = nullptr;   // SECONDS is optional, as --stats's
            const double v = i + 1 < argc ? std::strtod(argv[i + 1], &end) : 0.0;
            if (i + 1 < argc && end != argv[i + 1] && *end == 0 && v > 0) input_stats_seconds = v, i++;
        }
        else if (a == "--quiet") quiet = true;
        else if (a == "--mem-order") mem_order = true;
        else if (a == "--format" && i + 1 < argc) {
            const std::string f = argv[++i];
            cu8 = f == "cu8";
            if (f == "cu8") in_format = ADSB_DECIM_8BIT;
            else if (f == "cs16") in_format = ADSB_DECIM_CS16;
            else if (f == "cf32") in_format = ADSB_DECIM_CF32;
            else if (f == "s16real") in_format = ADSB_DECIM_REAL16;
            else path = nullptr, i = argc;
        }
        else if (a == "--fix" && i + 1 < argc) {
            const std::string f = argv[++i];
            if (f == "1bit") fix = ADSB_FIX_1BIT;
            else if (f == "2bit") fix = ADSB_FIX_2BIT;
            else if (f == "none") fix = ADSB_FIX_NONE;
            else path = nullptr, i = argc;
        }
        else if (a == "--help" || a == "-h") path = nullptr, i = argc;
        else path = argv[i];
    }
    // --shift: only in front of a filter, and only where a table of 256 entries at most does it
    const bool shift_ok = !shifted || ((decimate != 0) != (res_up != 0) &&
                                       adsb_mix_for_shift(decimate ? 1u : res_up, decimate ? (uint32_t)decimate : res_down, (int32_t)shift_hz,
                                                          &mix_k, &mix_period) == ADSB_OK);
    // --format cf32 | s16real: only in front of a filter (the scan's own entry points take neither); --scale: only with cf32
    const bool new_format = in_format == ADSB_DECIM_CF32 || in_format == ADSB_DECIM_REAL16;
    const bool format_ok = (!new_format || decimate || res_up) && (!scaled || in_format == ADSB_DECIM_CF32);
    // --input-stats: the statistics are a decimator's or a resampler's
    const bool input_stats_ok = !input_stats || decimate || res_up;
    if (!path || buffers < 1 || (decimate && res_up) || !shift_ok || !format_ok || !input_stats_ok) {
        std::fprintf(stderr, "usage: adsb_feed [--device N] [--port P] [--quiet] [--mem-order] [--format cs16|cu8|cf32|s16real] [--fix none|1bit|2bit] [--buffers K] [--latency-ms T] [--readers R] [--stats [SECONDS]] [--decimate D | --resample L/M] [--shift HZ] [--scale G] [--input-stats [SECONDS]] <capture.iq | ->\n");
        return 2;
    }
    std::signal(SIGPIPE, SIG_IGN);
    const int in = std::strcmp(path, "-") == 0 ? 0 : ::open(path, O_RDONLY);
    if (in < 0) {
        std::fprintf(stderr, "adsb_feed: cannot open %s: %s\n", path, std::strerror(errno));
        return 1;
    }
    Clients clients;
    if (port > 0 && !clients.listen_on(port)) {
        std::fprintf(stderr, "adsb_feed: cannot listen on port %d: %s\n", port, std::strerror(errno));
        return 1;
    }

    adsb_ctx *ctx = nullptr;
    int st = adsb_create(&ctx, device, (size_t)buffers);
    if (st != ADSB_OK) return die(nullptr, "adsb_create", st);
    if ((st = adsb_set_error_correction(ctx, fix)) != ADSB_OK) return die(ctx, "adsb_set_error_correction", st);
    if (stats && (st = adsb_set_signal_stats(ctx, 1)) != ADSB_OK) return die(ctx, "adsb_set_signal_stats", st);
    const size_t slot_samples = (size_t)buffers * ADSB_MODES_MAG_BUF_SAMPLES;
    const bool blocking = decimate || res_up;   // through the decimator or the resampler: the blocking call, not the ring
    if (!blocking && (st = cu8 ? adsb_ring_create_u8(ctx, slot_samples) : adsb_ring_create(ctx, slot_samples)) != ADSB_OK)
        return die(ctx, "adsb_ring_create", st);
    const size_t bps = in_format == ADSB_DECIM_CF32 ? 8 : in_format == ADSB_DECIM_CS16 ? 4 : 2;   // bytes per sample

    // a 112 us frame every 120 us would be ~450 per 55 ms buffer; neighbouring preamble
    // positions can each emit one, so leave an order of magnitude of room
    std::vector<adsb_msg> out(out_cap > 0 ? (size_t)out_cap : (size_t)buffers * 4096);
    unsigned long long total_samples = 0, total_frames = 0;
    SignalFold sig_interval, sig_total;
    std::vector<adsb_signal_stats> sig((size_t)buffers);
    auto t_stats = std::chrono::steady_clock::now();
    auto emit = [&](size_t n) {   // out[0, n) to stdout and to the clients
        std::string lines;
        char line[40];
        for (size_t i = 0; i < n; i++) {
            const int len = adsb_format_raw(&out[i], line, sizeof(line));
            if (len > 0) lines.append(line, (size_t)len);
        }
        total_frames += n;
        if (!quiet && !lines.empty()) {
            std::fwrite(lines.data(), 1, lines.size(), stdout);
            std::fflush(stdout);
        }
        clients.accept_new();
        if (!lines.empty()) clients.send_all(lines, latency_ms);
    };
    auto drain_one = [&]() -> int {
        size_t n = 0;
        int rc = adsb_collect(ctx, out.data(), out.size(), &n);
        if (rc == ADSB_ERR_CAPACITY) {  // more frames than the array holds: the context kept them all
            out.resize(n);
            rc = adsb_fetch_messages(ctx, out.data(), out.size(), &n);
        }
        if (rc != ADSB_OK) return rc;
        if (stats) {   // the pass's signal records: one per buffer (a pass never holds more than `buffers`)
            size_t n_sig = 0;
            if ((rc = adsb_fetch_signal_stats(ctx, sig.data(), sig.size(), &n_sig)) != ADSB_OK) return rc;
            for (size_t i = 0; i < n_sig; i++) sig_interval.add(sig[i]), sig_total.add(sig[i]);
            const auto now = std::chrono::steady_clock::now();
            if (std::chrono::duration<double>(now - t_stats).count() >= stats_seconds) {
                sig_interval.print("interval");
                sig_interval.clear();
                t_stats = now;
            }
        }
        emit(n);
        return ADSB_OK;
    };

    if (blocking) {
        // D x 2.4 MS/s, or 2.4 MS/s x M / L: whole calls of the input of `buffers` output buffers (--resample: of the
        // next multiple of L's odd part), so that the decimated or resampled stream is cut where consecutive reads of
        // 131072 samples of it would cut it
        int16_t taps[8 * 128 + 1];
        uint32_t n_taps = 0, shift = 0;
        adsb_decim *dec = nullptr;
        adsb_resamp *res = nullptr;
        size_t call_samples = 0;
        if (decimate) {
            if ((st = adsb_decim_default_taps((uint32_t)decimate, taps, sizeof(taps) / sizeof(taps[0]), &n_taps, &shift)) != ADSB_OK)
                return die(ctx, "adsb_decim_default_taps", st);
            if ((st = adsb_decim_create(ctx, (uint32_t)decimate, taps, n_taps, shift, &dec)) != ADSB_OK) return die(ctx, "adsb_decim_create", st);
            call_samples = slot_samples * (size_t)decimate;
        } else {
            if ((st = adsb_resamp_default_taps(res_up, res_down, taps, sizeof(taps) / sizeof(taps[0]), &n_taps, &shift)) != ADSB_OK)
                return die(ctx, "adsb_resamp_default_taps", st);
            if ((st = adsb_resamp_create(ctx, res_up, res_down, taps, n_taps, shift, &res)) != ADSB_OK) return die(ctx, "adsb_resamp_create", st);
            // 2.4 MS/s x M / L: K 131072 M / L inputs give K output buffers; a whole number where L's odd part divides K
            unsigned odd = res_up;
            while (odd % 2 == 0) odd /= 2;
            const size_t k = ((size_t)buffers + odd - 1) / odd * odd;
            call_samples = k * ADSB_MODES_MAG_BUF_SAMPLES / res_up * res_down;
            sig.resize(k);
            if (out_cap <= 0) out.resize(k * 4096);
        }
        const auto destroy = [&] { adsb_decim_destroy(dec), adsb_resamp_destroy(res); };
        if (shifted) {
            int16_t table[2 * ADSB_MIX_MAX_PERIOD];
            if ((st = adsb_mix_table(mix_k, mix_period, table, ADSB_MIX_MAX_PERIOD)) == ADSB_OK)
                st = dec ? adsb_mix_set_decim(dec, table, mix_period) : adsb_mix_set_resamp(res, table, mix_period);
            if (st != ADSB_OK) {
                destroy();
                return die(ctx, "adsb_mix_table / adsb_mix_set", st);
            }
        }
        if (scaled && (st = dec ? adsb_fmt_set_scale_decim(dec, scale) : adsb_fmt_set_scale_resamp(res, scale)) != ADSB_OK) {
            destroy();
            return die(ctx, "adsb_fmt_set_scale", st);
        }
        if (input_stats && (st = dec ? adsb_instat_set_decim(dec, 1) : adsb_instat_set_resamp(res, 1)) != ADSB_OK) {
            destroy();
            return die(ctx, "adsb_instat_set", st);
        }
        InputFold in_interval, in_total;
        auto t_input_stats = std::chrono::steady_clock::now();
        std::vector<char> in_buf(call_samples * bps);
        const auto t0 = std::chrono::steady_clock::now();
        for (bool eof = false; !eof;) {
            size_t fill = 0;
            while (!eof && fill < in_buf.size()) {
                bool idle = false;
                fill = read_once(in, in_buf.data(), fill, in_buf.size(), -1, &eof, &idle);
            }
            const size_t n_in = fill / bps;
            if (n_in == 0) break;
            if (!mem_order && in_format == ADSB_DECIM_CS16) swap_pairs(in_buf.data(), n_in);
            size_t n = 0;
            const int fmt = in_format;
            st = dec ? adsb_decim_demod_iq(dec, fmt, in_buf.data(), n_in, out.data(), out.size(), &n)
                     : adsb_resamp_demod_iq(res, fmt, in_buf.data(), n_in, out.data(), out.size(), &n);
            if (st == ADSB_ERR_CAPACITY) {
                out.resize(n);
                st = adsb_fetch_messages(ctx, out.data(), out.size(), &n);
            }
            if (st != ADSB_OK) {
                destroy();
                return die(ctx, dec ? "adsb_decim_demod_iq" : "adsb_resamp_demod_iq", st);
            }
            if (stats) {
                size_t n_sig = 0;
                if ((st = adsb_fetch_signal_stats(ctx, sig.data(), sig.size(), &n_sig)) != ADSB_OK) {
                    destroy();
                    return die(ctx, "adsb_fetch_signal_stats", st);
                }
                for (size_t i = 0; i < n_sig; i++) sig_total.add(sig[i]);
            }
            if (input_stats) {   // the call's record: the blocking call has finished, the fetch waits for nothing
                adsb_input_stats rec{};
                if ((st = dec ? adsb_instat_fetch_decim(dec, &rec) : adsb_instat_fetch_resamp(res, &rec)) != ADSB_OK) {
                    destroy();
                    return die(ctx, "adsb_instat_fetch", st);
                }
                in_interval.add(rec), in_total.add(rec);
                const auto now = std::chrono::steady_clock::now();
                if (std::chrono::duration<double>(now - t_input_stats).count() >= input_stats_seconds) {
                    in_interval.print("interval");
                    in_interval.clear();
                    t_input_stats = now;
                }
            }
            emit(n);
            total_samples += n_in;
        }
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (dec)
            std::fprintf(stderr, "adsb_feed: %llu samples at %d x 2.4 MS/s, %llu frames in %.3f s (%.1f Msamples/s); %llu clients dropped\n",
                         total_samples, decimate, total_frames, secs, secs > 0 ? total_samples / secs / 1e6 : 0.0, clients.dropped);
        else
            std::fprintf(stderr, "adsb_feed: %llu samples resampled by %u/%u to 2.4 MS/s, %llu frames in %.3f s (%.1f Msamples/s); %llu clients dropped\n",
                         total_samples, res_up, res_down, total_frames, secs, secs > 0 ? total_samples / secs / 1e6 : 0.0, clients.dropped);
        if (stats) sig_total.print("whole input");
        if (input_stats) in_total.print("whole input");
        if (in != 0) ::close(in);
        destroy();
        adsb_destroy(ctx);
        return 0;
    }

    struct stat sb{};
    const bool regular = in != 0 && ::fstat(in, &sb) == 0 && S_ISREG(sb.st_mode);
    FileFill file_fill(in, regular ? (readers < 1 ? 1 : readers > 16 ? 16 : readers) : 1, !mem_order && !cu8);
    off_t file_at = 0;

    const auto t_start = std::chrono::steady_clock::now();
    const size_t buf_bytes = (size_t)ADSB_MODES_MAG_BUF_SAMPLES * bps;
    std::vector<char> begun(buf_bytes);  // the buffer a short pass left unfinished: the next slot starts with it
    size_t begun_bytes = 0;
    unsigned long long short_passes = 0;
    bool eof = false;
    while (!eof) {
        void *buf = nullptr;
        size_t cap = 0;
        if (cu8) {
            uint8_t *b8 = nullptr;
            st = adsb_ring_acquire_u8(ctx, &b8, &cap);
            buf = b8;
        } else {
            int16_t *b16 = nullptr;
            st = adsb_ring_acquire(ctx, &b16, &cap);
            buf = b16;
        }
        if (st == ADSB_ERR_BUSY) {  // every slot in flight: finish the oldest first
            if ((st = drain_one()) != ADSB_OK) return die(ctx, "adsb_collect", st);
            continue;
        }
        if (st != ADSB_OK) return die(ctx, "adsb_ring_acquire", st);
        char *dst = (char *)buf;
        size_t fill = begun_bytes;
        if (fill) std::memcpy(dst, begun.data(), fill);
        begun_bytes = 0;
        // until the slot is full, the input ends, or latency_ms have gone by since the slot's first whole
        // buffer was complete (a deadline: data that keeps arriving does not put it off); meanwhile
        // finished passes are handed on and new clients accepted
        bool have_whole = fill >= buf_bytes;
        auto t_whole = std::chrono::steady_clock::now();
        if (regular) {   // all of it at once, by all the readers, swapped where it lands
            const size_t got = file_fill.fill(dst, file_at, cap * bps);
            file_at += (off_t)got;
            fill = got;
            eof = got < cap * bps;
            clients.accept_new();
        }
        while (!regular && !eof && fill < cap * bps) {
            int wait_ms = -1;   // nothing to hand on and no whole buffer yet: as long as it takes
            if (have_whole) {
                const long spent = (long)std::chrono::duration_cast<std::chrono::milliseconds>(
                                       std::chrono::steady_clock::now() - t_whole).count();
                if (spent >= latency_ms) break;   // a short pass
                wait_ms = (int)(latency_ms - spent);
            } else if (adsb_pending(ctx) > 0 || clients.listener >= 0) {
                wait_ms = latency_ms;
            }
            bool idle = false;
            fill = read_once(in, dst, fill, cap * bps, wait_ms, &eof, &idle);
            if (!have_whole && fill >= buf_bytes) {
                have_whole = true;
                t_whole = std::chrono::steady_clock::now();
            }
            clients.accept_new();
            if (idle && adsb_pending(ctx) > 0)  // idle input: do not sit on results
                if ((st = drain_one()) != ADSB_OK) return die(ctx, "adsb_collect", st);
        }
        size_t bytes = fill;
        if (!eof && fill < cap * bps) {  // short pass: whole buffers only, the begun one waits for its rest
            bytes = fill / buf_bytes * buf_bytes;
            begun_bytes = fill - bytes;
            std::memcpy(begun.data(), dst + bytes, begun_bytes);
            short_passes++;
        }
        const size_t n = bytes / bps;
        if (!mem_order && !cu8 && !regular) swap_pairs(dst, n);
        if (n == 0) break;
        if ((st = adsb_ring_submit(ctx, n)) != ADSB_OK) return die(ctx, "adsb_ring_submit", st);
        total_samples += n;
        clients.accept_new();
    }
    while (adsb_pending(ctx) > 0)
        if ((st = drain_one()) != ADSB_OK) return die(ctx, "adsb_collect", st);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    std::fprintf(stderr, "adsb_feed: %llu samples, %llu frames in %.3f s (%.1f Msamples/s); %llu short passes, %llu clients dropped\n",
                 total_samples, total_frames, secs, secs > 0 ? total_samples / secs / 1e6 : 0.0, short_passes, clients.dropped);
    if (stats) sig_total.print("whole input");
    if (in != 0) ::close(in);
    adsb_destroy(ctx);
    return 0;
}

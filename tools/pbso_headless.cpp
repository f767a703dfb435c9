// pbso_headless -- headless counterpart of the reference's GUI tool for the hot path.
//
// Takes the reference's command-line flags (tools/real_time_modal_sound.cpp:42-64:
// -d/--data_dir, -name/--obj_name, -m/--mesh, -s/--surf_mode, -t/--material,
// -p/--ffat_map) and its directory convention (:480-501), builds the solver the way
// BuildSolver does (:309-345) through the C ABI, replaces the mouse by a hit script and
// the camera by a listener script, steps N buffers on the MI355X and writes what
// PaModalCallback would have played (:207-210, sound / 1e10) as a mono float32 WAV.
//
//   --hits FILE      lines: <buffer> <vertex_id> <nx> <ny> <nz> [point|gauss <width_us>|ar]
//                    or:    <buffer> <vertex_id> - [point|gauss <width_us>|ar]   (normal = VN.row(vid) of the mesh:
//                    igl::per_vertex_normals of the .obj, tools/...:509,607 -- needs -m / -d)
//   --listener FILE  lines: <buffer> <x> <y> <z>          (computeTransfer at that buffer)
//   --strokes FILE   sustained contact (the mouse dragged over the surface, tools/...:754-776, 1127-1160), lines:
//                    <buffer> <v0> <v1> <v2> <c0> <c1> <c2> <nx> <ny> <nz> [start|end]   a GetModalForceFace message (vn as given)
//                    <buffer> - [start|end]                                              the dummy start / stop message (setZero(N))
//                    fed one step ahead through pbso_enqueue_strokes (with --devices: to the engines of the ranks);
//                    --stroke-force point|ar (default ar);  --arprm "<a0> <a1> <sigma> <mu>"  AR parameters from buffer 0 on
//   --track-hits FILE  hits whose force is a caller-supplied signal (pbso_enqueue_track_force), lines:
//                    <buffer> <start_sample> <vertex_id> <nx> <ny> <nz> <track file> [gain [rate [first [n_samples [loop]]]]]
//                    (`-` for the normal as in --hits); the force starts at in-buffer sample <start_sample> of that buffer.  A track
//                    file is raw little-endian float32 (.f32) or a mono IEEE-float WAV such as this tool writes; every distinct
//                    path is loaded once.  Composes with --hits (one queue, in buffer order; at equal buffers the --hits line first)
//   --buffers N      number of 513-sample buffers (default 86 ~ 1 s)
//   --out FILE       output WAV (default out.wav);  --raw FILE also dumps the fp32 sound values
//   --devices 0,1,.. several GPUs through the C ABI's device group (one engine per GPU, objects sharded by the sum of their
//                    modes, RCCL only for the final collective): the scene is --copies K instances of the object (default: one
//                    per device), copy c hears the hit and listener scripts c * --copy-shift buffers later (default 1), and
//                    the WAV is their MIX (PBSO_GATHER_MIX: every GPU sums its objects, the GPUs all-reduce one row)
//   --channels C --pan FILE [--ramp N]   a C-channel scene mix (pbso_scene_mix; with --devices PBSO_GATHER_SCENE) instead of the
//                    mono one: lines <buffer> <copy> <g_0> <d_0> ... <g_{C-1}> <d_{C-1}> set copy's gain and delay (samples) per
//                    channel from that buffer on, ramped over N samples (default 441); the tool steps the segments between
//                    these change points, mixes each, and writes a C-channel interleaved float32 WAV (--raw: the same frames)
//   --pan-schedule   with --pan: the pan lines are scheduled up front at sample <buffer> * frames (pbso_scene_mix_set_at; with
//                    --devices pbso_group_scene_mix_set_at) and no longer cut the run -- the same samples in the WAV, in one step
//                    unless another script (--retune) cuts it
//   --time-chunks N  pbso_engine_desc::time_chunks for every engine (0, the default: the engine's policy; N > 0: every launch cut
//                    along the time axis, N buffers per chunk; < 0: never).  With N = 1 the samples do not depend, to the last
//                    bit, on how a script cuts the run into steps: a run with --pan-schedule is then byte for byte the run without
//   --channels C --fir FILE [--xfade N]  the same through the scene filter mix (pbso_scene_fir; with --devices PBSO_GATHER_FIR):
//                    lines <buffer> <copy> <onset> <taps file> give copy a filter per channel behind an onset (samples) from that
//                    buffer on, cross-faded over N samples (default 441; change points must be at least that far apart).  A taps
//                    file is raw little-endian float32 [C][K], every file with the same K; every distinct path is loaded once.
//                    Not together with --pan.
//   --channels C --fir-bank FILE --fir-taps K --fir-dirs SCRIPT   in place of --fir: the filters come from a bank that is uploaded
//                    once (pbso_scene_fir_bank_create) -- FILE is raw little-endian float32 [F][C][K], F follows from its size --
//                    and SCRIPT's lines <buffer> <copy> <onset> <i0> <w0> [<i1> <w1> ... up to 8 pairs] give copy the filter
//                    sum_j w_j * bank[i_j] (one fmaf per pair, in the line's order) from that buffer on.  A line with fewer
//                    pairs than the script's widest is padded with (0, 0.f), which adds nothing.  Composes with --xfade,
//                    --fir-delay, --fir-schedule, --reverb, --limit, --out-rate and --devices exactly as --fir does; not
//                    together with --fir or --pan.
//   --fir-delay FILE [--delay-ramp N]    with --fir: the filter mix's delay stage (pbso_scene_fir_delay_enable): lines <buffer> <copy>
//                    <delay in samples> set copy's fractional delay in front of its filters from that buffer on, ramped over N
//                    samples (default 441; a moving source's Doppler shift).  max_delay is the file's largest value, rounded
//                    up; the run is cut at these lines' buffers too.
//   --fir-schedule   with --fir (and --fir-delay when given): all lines are scheduled up front at sample <buffer> * frames
//                    (pbso_scene_fir_set_at / _set_delay_at; with --devices the group's calls) and no longer cut the run -- the
//                    same samples in the WAV (byte for byte with --time-chunks 1 on both commands), in one step unless another
//                    script (--retune) cuts it
//   --reverb FILE [--reverb-xfade N]     with --channels C and one of --pan / --fir: the room behind the mix (pbso_scene_reverb).  The
//                    file is an impulse response per output channel, raw little-endian float32 [C][K], K = file size / 4 C up to
//                    131072; the send bus is the object mix (pbso_mix_objects, one input), and the WAV is dry + wet: every
//                    segment's mix goes in as d_add.  N is the reverb's cross-fade length (default 441).  One engine only: not
//                    with --devices (the wet signal of an all-reduced bus is not the bitwise sum of per-rank wet signals).
//   --limit T [--lookahead L] [--hold H] [--gain G] [--pcm16]   the master bus (pbso_master) behind whatever the tool would have
//                    written -- the mono object mix, --pan, --fir, or dry + wet with --reverb: the samples of the WAV without
//                    --limit times G (default 1) through the look-ahead limiter with ceiling T (0 < T <= 1), look-ahead L
//                    (default 64, 1 .. 4096) and hold H (default 0).  The limiter delays by L samples: the tool steps ceil(L / 513)
//                    more buffers with no hits, so that the objects' own tail fills them, and drops the first L output samples:
//                    the file has the length and alignment of the run without --limit.  --pcm16 writes a 16-bit PCM WAV (format 1)
//                    converted on the device (pbso_read_master_pcm16); only with --limit.  One engine only: not with --devices;
//                    not with --raw (the unscaled mix).
//   --out-rate R [--rs-taps T] [--rs-beta B] [--rs-cutoff F]   the resampler bus (pbso_resample) behind whatever the tool would have
//                    written -- the mono object mix, --pan, --fir, dry + wet with --reverb, and --limit's output when that is given:
//                    the WAV's samples at R Hz instead of 44100, through T taps per output sample (default 32, 1 .. 256) of a
//                    Kaiser-windowed sinc (beta B, default 9; cutoff F, default 0.9).  The WAV header carries R.  The converter
//                    delays by (L T - 1) / (2 L) input samples (L = R / gcd(R, 44100)): with d = that plus --limit's look-ahead,
//                    the tool steps enough more buffers with no hits to flush d, drops the first floor(d L / M + 0.5) output
//                    frames and writes ceil(buffers * 513 * L / M) of them.  --pcm16 beside it takes the resampler's saturating
//                    PCM (pbso_read_resample_pcm16) and still needs --limit.  One engine only: not with --devices; not with --raw.
//   --eq FILE [--eq-xfade N]   with --channels C and one of --pan / --fir: the EQ bus (pbso_eq) behind the mixers and the reverb and in
//                    front of --limit and --out-rate, on the samples of the WAV without it.  Lines <buffer> <section> <kind> <f0>
//                    <Q> <gain dB> give section 0 .. 7 of every channel the cookbook design (pbso_eq_design; kind lowpass, highpass,
//                    peak, lowshelf or highshelf) from that buffer on; the sections not named yet pass the signal through.  The run
//                    is cut at these buffers as --pan cuts it; a buffer's lines are one set, cross-faded over N samples (default
//                    441; a fade must be over before the next set, else the run ends with the engine's refusal).  One engine only:
//                    not with --devices; not with --raw.
//   --eq-schedule    with --eq: every line is scheduled up front at sample <buffer> * frames (pbso_eq_set_at; a buffer's lines are
//                    one set) and the lines no longer cut the run.  The same samples in the WAV (byte for byte with --time-chunks 1
//                    on both commands).  The schedule's spacing rule holds from sample 0 on: lines closer than the fade allows, a
//                    first line before sample N - 1 among them, are refused before anything runs.
//   --loudness FILE [--loudness-target T]   the loudness bus (pbso_loudness) on what the tool writes, at the engine's rate: the mono
//                    object mix, --pan, --fir, dry + wet with --reverb, behind --eq when that is given.  FILE gets `key value` lines,
//                    %.17g: the report of pbso_loudness_report (integrated, momentary, short_term, max_momentary, max_short_term,
//                    relative_threshold in LUFS; true_peak and sample_peak linear; n_blocks, n_gated), target and gain_to_target =
//                    pow(10, (T - integrated) / 20) (T in LUFS, default -23), then every record of the log as energy.<j>.<c>,
//                    true_peak.<j>.<c>, sample_peak.<j>.<c>.  Only whole sub-blocks of 100 ms count.  The workflow is: measure, then
//                    render again with --limit ... --gain G.  One engine only: not with --devices; not with --limit, --out-rate
//                    (it would measure in front of them) or --raw.
//   --retune FILE    materials changed during the run (pbso_set_material; with --devices pbso_group_set_material): lines
//                    <buffer> <copy> <material file> [keep|zero] give copy the file's material (the format of -t) from that
//                    buffer on; keep (the default): the state carries on under the new coefficients, zero: it is cleared.  Every
//                    distinct path is loaded once.  The run is cut at these buffers as --pan cuts it; composes with --copies,
//                    --channels and --limit.  The mode count stays the one of the -t material.
#include <dirent.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "openpbso_amd.h"
#include "resample_clock.h"                              // (openpbso_amd/csrc: the resampler's limits and counts, no HIP in it)
#include "eq_schedule.h"                                 // (... and its schedule's spacing rule)
#include "eq_block.h"                                    // (openpbso_amd/csrc: the EQ bus's limits and refusals, no HIP in it)
#include "loudness_gate.h"                               // (openpbso_amd/csrc: the loudness bus's hop, no HIP in it)

static void die(const std::string &msg) {
    std::fprintf(stderr, "pbso_headless: %s\n", msg.c_str());
    std::exit(1);
}
static void check(pbso_engine *e, int rc, const char *what) {
    if (rc < 0) die(std::string(what) + ": " + pbso_status_string(rc) + ": " + (e ? pbso_last_error(e) : ""));
}

// ListDirFiles(d, names, ".tet.obj") + Basename + prefix up to the first '.', tools/...:483-487
static std::string guess_name(const std::string &dir) {
    DIR *d = opendir(dir.c_str());
    if (!d) die("cannot open data dir " + dir);
    std::string found;
    while (dirent *ent = readdir(d)) {
        const std::string f = dir + "/" + ent->d_name;
        if (ent->d_name[0] != '.' && f.find(".tet.obj") != std::string::npos) { found = ent->d_name; break; }
    }
    closedir(d);
    if (found.empty()) die("no *.tet.obj in " + dir);
    return found.substr(0, found.find_first_of("."));
}

static void write_wav_f32(const std::string &path, const std::vector<float> &mono, int rate, int channels = 1) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) die("cannot write " + path);
    const uint32_t data_bytes = (uint32_t)(mono.size() * 4), riff = 36 + data_bytes, fmt_len = 16, byte_rate = rate * 4 * channels;
    const uint16_t fmt = 3 /* IEEE float */, ch = (uint16_t)channels, align = (uint16_t)(4 * channels), bits = 32;
    const uint32_t r = rate;
    std::fwrite("RIFF", 1, 4, f); std::fwrite(&riff, 4, 1, f); std::fwrite("WAVEfmt ", 1, 8, f);
    std::fwrite(&fmt_len, 4, 1, f); std::fwrite(&fmt, 2, 1, f); std::fwrite(&ch, 2, 1, f);
    std::fwrite(&r, 4, 1, f); std::fwrite(&byte_rate, 4, 1, f); std::fwrite(&align, 2, 1, f); std::fwrite(&bits, 2, 1, f);
    std::fwrite("data", 1, 4, f); std::fwrite(&data_bytes, 4, 1, f);
    std::fwrite(mono.data(), 4, mono.size(), f);
    std::fclose(f);
}

static void write_wav_pcm16(const std::string &path, const std::vector<int16_t> &frames, int rate, int channels) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) die("cannot write " + path);
    const uint32_t data_bytes = (uint32_t)(frames.size() * 2), riff = 36 + data_bytes, fmt_len = 16, byte_rate = rate * 2 * channels;
    const uint16_t fmt = 1 /* PCM */, ch = (uint16_t)channels, align = (uint16_t)(2 * channels), bits = 16;
    const uint32_t r = rate;
    std::fwrite("RIFF", 1, 4, f); std::fwrite(&riff, 4, 1, f); std::fwrite("WAVEfmt ", 1, 8, f);
    std::fwrite(&fmt_len, 4, 1, f); std::fwrite(&fmt, 2, 1, f); std::fwrite(&ch, 2, 1, f);
    std::fwrite(&r, 4, 1, f); std::fwrite(&byte_rate, 4, 1, f); std::fwrite(&align, 2, 1, f); std::fwrite(&bits, 2, 1, f);
    std::fwrite("data", 1, 4, f); std::fwrite(&data_bytes, 4, 1, f);
    std::fwrite(frames.data(), 2, frames.size(), f);
    std::fclose(f);
}

struct Hit { long b; pbso_force_msg m; int track = -1; pbso_track_play play; };   // track >= 0: a --track-hits line, index into the tracks
struct Pos { long b; double p[3]; };
// a track file: raw little-endian float32, or a mono IEEE-float WAV (the chunks walked; `fmt ` format 3, 32 bits, one channel)
static std::vector<float> read_track_file(const std::string &path) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) die("cannot read track " + path);
    std::vector<unsigned char> bytes;
    unsigned char buf[1 << 16];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
    size_t off = 0, len = bytes.size();
    const bool wav = path.size() >= 4 && (path.compare(path.size() - 4, 4, ".wav") == 0 || path.compare(path.size() - 4, 4, ".WAV") == 0);
    if (wav) {
        auto u32 = [&](size_t o) { return (uint32_t)bytes[o] | (uint32_t)bytes[o + 1] << 8 | (uint32_t)bytes[o + 2] << 16 | (uint32_t)bytes[o + 3] << 24; };
        auto u16 = [&](size_t o) { return (unsigned)(bytes[o] | bytes[o + 1] << 8); };
        if (bytes.size() < 12 || std::memcmp(bytes.data(), "RIFF", 4) != 0 || std::memcmp(bytes.data() + 8, "WAVE", 4) != 0) die("not a WAV file: " + path);
        bool have_fmt = false, have_data = false;
        for (size_t o = 12; o + 8 <= bytes.size();) {
            const size_t n = u32(o + 4);
            if (o + 8 + n > bytes.size()) die("truncated WAV chunk: " + path);
            if (std::memcmp(bytes.data() + o, "fmt ", 4) == 0) {
                if (n < 16 || u16(o + 8) != 3 || u16(o + 10) != 1 || u16(o + 22) != 32) die("track WAV must be mono IEEE float32: " + path);
                have_fmt = true;
            } else if (std::memcmp(bytes.data() + o, "data", 4) == 0) {
                off = o + 8; len = n; have_data = true;
                break;
            }
            o += 8 + n + (n & 1);
        }
        if (!have_fmt || !have_data) die("WAV without fmt / data chunk: " + path);
    }
    if (len < 4 || len % 4 != 0) die("track file holds no whole float32 samples: " + path);
    std::vector<float> out(len / 4);
    std::memcpy(out.data(), bytes.data() + off, len);
    return out;
}
// one message into engine e: a --hits line through pbso_enqueue_force, a --track-hits line with its play record
static int enqueue_hit(pbso_engine *e, int obj, const Hit &h, const std::vector<int> &track_ids, long stamp) {
    if (h.track < 0) return pbso_enqueue_force(e, obj, &h.m, stamp);
    pbso_track_play play = h.play;
    play.track = track_ids[(size_t)h.track];
    return pbso_enqueue_track_force(e, obj, &h.m, &play, stamp);
}
static std::vector<int> create_tracks(pbso_engine *e, const std::vector<std::vector<float>> &tracks) {
    std::vector<int> ids(tracks.size(), -1);
    for (size_t t = 0; t < tracks.size(); ++t) check(e, pbso_track_create(e, tracks[t].data(), (int64_t)tracks[t].size(), &ids[t]), "track_create");
    return ids;
}

// --strokes: one entry of the script, and the arrays one pbso_enqueue_strokes call borrows until its step returns
struct Stroke { long b; unsigned char flags; int v[3]; double c[3], n[3]; };
struct StrokeFeed {
    std::vector<int> objs, vids;
    std::vector<double> coords, vn;
    std::vector<int64_t> stamps;
    std::vector<unsigned char> flags;
};
struct StrokeScript {
    std::vector<Stroke> entries;                 // ascending buffers
    int force_type = PBSO_AUTOREGRESSIVE_FORCE;
    bool have_arprm = false;
    double arprm[4] = {0, 0, 0, 0};
};
// the entries of buffers [b0, b1) for the objects `ids` (ascending) of engine e, object ids[k] hearing the script shift[k] buffers later
static void feed_strokes(pbso_engine *e, const StrokeScript &sc, const std::vector<int> &ids, const std::vector<long> &shift, long b0, long b1,
                         StrokeFeed &f) {
    f = StrokeFeed();
    for (size_t k = 0; k < ids.size(); ++k)
        for (const Stroke &s : sc.entries) {
            const long b = s.b + shift[k];
            if (b < b0 || b >= b1) continue;
            f.objs.push_back(ids[k]);
            f.stamps.push_back(b);
            f.flags.push_back(s.flags);
            for (int j = 0; j < 3; ++j) { f.vids.push_back(s.v[j]); f.coords.push_back(s.c[j]); f.vn.push_back(s.n[j]); }
        }
    if (f.objs.empty()) return;
    const int rc = pbso_enqueue_strokes(e, (int)f.objs.size(), f.objs.data(), f.vids.data(), f.coords.data(), f.vn.data(), f.stamps.data(),
                                        f.flags.data(), sc.force_type);
    check(e, rc, "enqueue_strokes");
}
// --channels / --pan: the scene mix's script
struct Pan { long b; int copy; std::vector<float> gd; };   // gd: g_0 d_0 ... g_{C-1} d_{C-1}
struct FirLine { long b; int copy, onset, file; std::vector<std::pair<int, float>> pairs; };   // file: index into Scene::fir_files; pairs: --fir-dirs
struct FirDelayLine { long b; int copy; float delay; };     // --fir-delay: <buffer> <copy> <delay in samples>
struct Scene {
    int channels = 0, ramp = 441, copies = 1, max_delay = 0;
    std::vector<Pan> lines;
    bool pan_schedule = false;                           // --pan-schedule: the lines are scheduled up front and cut nothing
    // --fir: the scene filter mix's script instead of the pan script
    bool fir = false;
    bool fir_schedule = false;                           // --fir-schedule: the --fir and --fir-delay lines are scheduled up front and cut nothing
    int xfade = 441, n_taps = 0, max_onset = 0;
    std::vector<FirLine> fir_lines;
    std::vector<std::vector<float>> fir_files;           // [C][K] each
    // --fir-bank / --fir-dirs: the filters stay on the device and a line names (index, weight) pairs into them; a copy's pairs as
    // last set, [copies][bank_J] (a line with fewer pairs than the widest is padded with (0, 0.f), which adds nothing)
    bool fir_bank = false;
    std::vector<float> bank;                             // [bank_F][C][K]
    int bank_F = 0, bank_J = 0;
    mutable std::vector<int> bank_index;
    mutable std::vector<float> bank_weight;
    // --fir-delay: the filter mix's delay stage (a ramped fractional delay per copy in front of the filters)
    std::vector<FirDelayLine> fir_delay_lines;
    int fir_max_delay = 0, fir_delay_ramp = 441;
    // --reverb: an impulse response [C][reverb_taps] behind either mixer
    std::vector<float> reverb;
    int reverb_taps = 0, reverb_xfade = 441;
    // segments [cuts[k], cuts[k + 1]) between the change points; set_at(b) updates gain / delay [C][copies] for buffer b
    std::vector<int> cuts(int n_buffers) const {
        std::vector<int> c{0, n_buffers};
        for (const Pan &p : lines)
            if (!pan_schedule && p.b > 0 && p.b < n_buffers) c.push_back((int)p.b);
        for (const FirLine &p : fir_lines)
            if (!fir_schedule && p.b > 0 && p.b < n_buffers) c.push_back((int)p.b);
        for (const FirDelayLine &p : fir_delay_lines)
            if (!fir_schedule && p.b > 0 && p.b < n_buffers) c.push_back((int)p.b);
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        return c;
    }
    bool set_at(long b, std::vector<float> &gain, std::vector<float> &delay) const {
        bool any = false;
        for (const Pan &p : lines)
            if (p.b == b) {
                for (int c = 0; c < channels; ++c) {
                    gain[(size_t)c * copies + p.copy] = p.gd[2 * c];
                    delay[(size_t)c * copies + p.copy] = p.gd[2 * c + 1];
                }
                any = true;
            }
        return any;
    }
    // --pan-schedule: every buffer that has pan lines, in order, as one set at its first sample: set(t_set, gain, delay)
    template <class Set>
    void schedule_pan(std::vector<float> &gain, std::vector<float> &delay, Set set) const {
        std::vector<long> at;
        for (const Pan &p : lines) at.push_back(p.b);
        std::sort(at.begin(), at.end());
        at.erase(std::unique(at.begin(), at.end()), at.end());
        for (long b : at)
            if (set_at(b, gain, delay)) set((int64_t)b * PBSO_FRAMES_PER_BUFFER, gain.data(), delay.data());
    }
    // ... and taps [C][copies][K] (--fir-dirs: bank_index / bank_weight instead), onset [copies]
    bool fir_set_at(long b, std::vector<float> &taps, std::vector<int> &onset) const {
        bool any = false;
        for (const FirLine &p : fir_lines)
            if (p.b == b) {
                for (int j = 0; fir_bank && j < bank_J; ++j) {
                    bank_index[(size_t)p.copy * bank_J + j] = j < (int)p.pairs.size() ? p.pairs[j].first : 0;
                    bank_weight[(size_t)p.copy * bank_J + j] = j < (int)p.pairs.size() ? p.pairs[j].second : 0.f;
                }
                for (int c = 0; !fir_bank && c < channels; ++c)
                    std::copy(fir_files[p.file].begin() + (size_t)c * n_taps, fir_files[p.file].begin() + (size_t)(c + 1) * n_taps,
                              taps.begin() + ((size_t)c * copies + p.copy) * n_taps);
                onset[p.copy] = p.onset;
                any = true;
            }
        return any;
    }
    // ... and delay [copies]
    bool fir_delay_set_at(long b, std::vector<float> &delay) const {
        bool any = false;
        for (const FirDelayLine &p : fir_delay_lines)
            if (p.b == b) {
                delay[p.copy] = p.delay;
                any = true;
            }
        return any;
    }
    // --fir-schedule: every buffer that has --fir lines, in order, as one set at its first sample: set(t_set, taps, onset); and the
    // same for the --fir-delay lines: set_delay(t_set, delay)
    template <class Set, class SetDelay>
    void schedule_fir(std::vector<float> &taps, std::vector<int> &onset, std::vector<float> &delay, Set set, SetDelay set_delay) const {
        std::vector<long> at, at_delay;
        for (const FirLine &p : fir_lines) at.push_back(p.b);
        for (const FirDelayLine &p : fir_delay_lines) at_delay.push_back(p.b);
        for (std::vector<long> *v : {&at, &at_delay}) {
            std::sort(v->begin(), v->end());
            v->erase(std::unique(v->begin(), v->end()), v->end());
        }
        for (long b : at)
            if (fir_set_at(b, taps, onset)) set((int64_t)b * PBSO_FRAMES_PER_BUFFER, taps.data(), onset.data());
        for (long b : at_delay)
            if (fir_delay_set_at(b, delay)) set_delay((int64_t)b * PBSO_FRAMES_PER_BUFFER, delay.data());
    }
};

// --retune: the material script.  Lines <buffer> <copy> <material file> [keep|zero]: from that buffer on the copy has the file's
// material (pbso_set_material; keep, the default: the state carries on, zero: it is cleared).  The run is cut at these buffers.
struct RetuneLine { long b; int copy, file; bool keep; };
struct RetuneScript {
    std::vector<RetuneLine> lines;
    std::vector<std::string> paths;                      // every distinct material file, loaded once
    std::vector<pbso_material> materials;
    bool empty() const { return lines.empty(); }
    void read(const std::string &path, int copies, int n_buffers) {
        std::ifstream f(path);
        if (!f) die("cannot read " + path);
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::istringstream iss(line);
            RetuneLine p;
            std::string file, word;
            if (!(iss >> p.b >> p.copy >> file)) die("bad retune line (<buffer> <copy> <material file> [keep|zero]): " + line);
            p.keep = true;
            if (iss >> word) {
                if (word == "zero") p.keep = false;
                else if (word != "keep") die("bad retune line (keep or zero): " + line);
            }
            if (p.copy < 0 || p.copy >= copies) die("retune line for a copy that does not exist: " + line);
            if (p.b < 0 || p.b >= n_buffers) die("retune line outside buffers 0 .. --buffers - 1: " + line);
            p.file = (int)(std::find(paths.begin(), paths.end(), file) - paths.begin());
            if (p.file == (int)paths.size()) {
                double mat[5];
                if (pbso_material_read(file.c_str(), mat) != PBSO_OK) die("cannot read material file " + file);
                paths.push_back(file);
                materials.push_back(pbso_material{mat[0], mat[3], mat[4]});
            }
            lines.push_back(p);
        }
        if (lines.empty()) die("no lines in " + path);
    }
    // the change points merged into a list of cuts (sorted, unique; the last entry stays the end of the run)
    std::vector<int> cut(std::vector<int> cuts, int n_buffers) const {
        for (const RetuneLine &p : lines)
            if (p.b > 0 && p.b < n_buffers) cuts.push_back((int)p.b);
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        return cuts;
    }
    // the lines of buffer b as one call per keep / zero: set(n, copies, materials, keep_state)
    template <class Set>
    void apply_at(long b, Set set) const {
        for (int keep = 1; keep >= 0; --keep) {
            std::vector<int> ids;
            std::vector<pbso_material> mats;
            for (const RetuneLine &p : lines)
                if (p.b == b && p.keep == (keep != 0)) {
                    // (a copy named twice at one buffer: the later line wins, as a later buffer's would)
                    auto at = std::find(ids.begin(), ids.end(), p.copy);
                    if (at != ids.end()) mats[at - ids.begin()] = materials[p.file];
                    else { ids.push_back(p.copy); mats.push_back(materials[p.file]); }
                }
            if (!ids.empty()) set((int)ids.size(), ids.data(), mats.data(), keep);
        }
    }
};

// the scene on several GPUs (include/openpbso_amd.h "device group")
static int run_group(const std::vector<int> &devices, int copies, int shift, const std::string &modes, const std::string &material,
                     const std::string &ffat, const std::vector<Hit> &hits, const std::vector<std::vector<float>> &tracks,
                     const std::vector<Pos> &path, const StrokeScript &strokes, int n_buffers, const Scene *scene, const RetuneScript &retune, int time_chunks,
                     std::vector<float> &sound) {
    auto gcheck = [](pbso_group *g, int rc, const char *what) {
        if (rc < 0) die(std::string(what) + ": " + pbso_status_string(rc) + ": " + (g ? pbso_group_last_error(g) : ""));
    };
    // BuildSolver's inputs (tools/...:309-345), read once: the audible mode count is what the shards are balanced by
    double mat[5];
    if (pbso_material_read(material.c_str(), mat) != PBSO_OK) die("cannot read material file " + material);
    int n_dof = 0, n_modes = 0;
    double *om = nullptr, *md = nullptr;
    if (pbso_modes_read(modes.c_str(), &n_dof, &n_modes, &om, &md) != PBSO_OK) die("cannot read modes " + modes);
    double max_freq = 20000.;                            // tools/...:316-329
    if (!ffat.empty()) {
        std::ifstream f((ffat + "/freq_threshold.txt").c_str());
        if (f) f >> max_freq;
    }
    const int n_aud = pbso_num_modes_audible(om, n_modes, mat[0], max_freq);
    pbso_group_desc gd;
    std::memset(&gd, 0, sizeof(gd));
    gd.abi_version = PBSO_ABI_VERSION;
    gd.devices = devices.data();
    gd.n_devices = (int)devices.size();
    gd.engine.abi_version = PBSO_ABI_VERSION;
    gd.engine.qnorm_mode = PBSO_QNORM_OFF;
    gd.engine.time_chunks = time_chunks;
    pbso_group *g = nullptr;
    gcheck(g, pbso_group_create(&gd, &g), "group_create");
    std::vector<int> mc(copies, n_aud);
    gcheck(g, pbso_group_plan(g, mc.data(), copies), "group_plan");
    pbso_object_desc od;
    std::memset(&od, 0, sizeof(od));
    od.n_modes = n_aud; od.n_omega = n_modes; od.omega_squared = om;
    od.density = mat[0]; od.alpha = mat[3]; od.beta = mat[4];
    od.n_dof = n_dof; od.mode_shapes = md;
    for (int c = 0; c < copies; ++c) {
        gcheck(g, pbso_group_add_object(g, c, &od), "group_add_object");
        int rank = 0, local = 0;
        gcheck(g, pbso_group_owner(g, c, &rank, &local), "group_owner");
        pbso_engine *e = pbso_group_engine(g, rank);
        if (e && !ffat.empty()) check(e, pbso_object_read_ffat_maps(e, local, ffat.c_str()), "read_ffat_maps");
    }
    pbso_free(om);
    pbso_free(md);
    gcheck(g, pbso_group_finalize(g), "group_finalize");
    std::vector<std::vector<int>> rank_tracks(devices.size());     // the tracks once per engine that owns a copy
    for (int c = 0; c < copies; ++c) {
        int rank = 0, local = 0;
        gcheck(g, pbso_group_owner(g, c, &rank, &local), "group_owner");
        pbso_engine *e = pbso_group_engine(g, rank);
        if (path.empty()) check(e, pbso_set_use_transfer(e, local, 0, 0), "set_use_transfer");
        for (const Pos &p : path) check(e, pbso_compute_transfer(e, local, p.p, p.b + (long)c * shift), "compute_transfer");
        if (!tracks.empty() && rank_tracks[rank].empty()) rank_tracks[rank] = create_tracks(e, tracks);
        for (const Hit &h : hits) {
            int rc;
            if (h.track < 0) {
                rc = pbso_group_enqueue_force(g, c, &h.m, h.b + (long)c * shift);
                gcheck(g, rc, "group_enqueue_force");
            } else {
                rc = enqueue_hit(e, local, h, rank_tracks[rank], h.b + (long)c * shift);
                check(e, rc, "enqueue_track_force");
            }
            if (rc == 0) die("force queue full");
        }
        if (strokes.have_arprm) check(e, pbso_enqueue_arprm(e, local, strokes.arprm, strokes.arprm[2], strokes.arprm[3], (long)c * shift), "enqueue_arprm");
    }
    // the stroke script goes to the engines of the ranks, every rank its own copies (ascending local ids), step by step
    std::vector<std::vector<int>> rank_ids(devices.size());
    std::vector<std::vector<long>> rank_shift(devices.size());
    for (int c = 0; c < copies && !strokes.entries.empty(); ++c) {
        int rank = 0, local = 0;
        gcheck(g, pbso_group_owner(g, c, &rank, &local), "group_owner");
        auto at = std::lower_bound(rank_ids[rank].begin(), rank_ids[rank].end(), local) - rank_ids[rank].begin();
        rank_ids[rank].insert(rank_ids[rank].begin() + at, local);
        rank_shift[rank].insert(rank_shift[rank].begin() + at, (long)c * shift);
    }
    std::vector<StrokeFeed> feeds(devices.size());
    auto feed_ranks = [&](long b0, long b1) {
        for (size_t r = 0; r < devices.size(); ++r)
            if (!rank_ids[r].empty()) feed_strokes(pbso_group_engine(g, (int)r), strokes, rank_ids[r], rank_shift[r], b0, b1, feeds[r]);
    };
    auto group_set = [&](int n, const int *ids, const pbso_material *mats, int keep) {
        gcheck(g, pbso_group_set_material(g, n, ids, mats, keep), "group_set_material");
    };
    if (scene) {
        // the segments between the pan script's change points, each gathered as a C-channel scene mix: sound [C][n_buffers * B]
        const int C = scene->channels;
        const size_t total = (size_t)n_buffers * PBSO_FRAMES_PER_BUFFER;
        if (scene->fir) gcheck(g, pbso_group_scene_fir_enable(g, C, scene->n_taps, scene->max_onset, scene->xfade), "group_scene_fir_enable");
        else gcheck(g, pbso_group_scene_mix_enable(g, C, scene->max_delay, scene->ramp), "group_scene_mix_enable");
        if (scene->fir_bank) gcheck(g, pbso_group_scene_fir_bank_create(g, scene->bank_F, scene->bank.data()), "group_scene_fir_bank_create");
        if (!scene->fir_delay_lines.empty())
            gcheck(g, pbso_group_scene_fir_delay_enable(g, scene->fir_max_delay, scene->fir_delay_ramp), "group_scene_fir_delay_enable");
        std::vector<float> fir_delay(copies, 0.f);
        std::vector<float> gain((size_t)C * copies, 0.f), delay((size_t)C * copies, 0.f), seg;
        std::vector<float> taps(scene->fir ? (size_t)C * copies * scene->n_taps : 0, 0.f);
        std::vector<int> onset(copies, 0);
        sound.assign((size_t)C * total, 0.f);
        if (scene->pan_schedule)
            scene->schedule_pan(gain, delay, [&](int64_t t, const float *gn, const float *dl) {
                gcheck(g, pbso_group_scene_mix_set_at(g, t, gn, dl), "group_scene_mix_set_at");
            });
        if (scene->fir_schedule)
            scene->schedule_fir(taps, onset, fir_delay,
                                [&](int64_t t, const float *h, const int *on) {
                                    if (scene->fir_bank)
                                        gcheck(g, pbso_group_scene_fir_set_bank_at(g, t, scene->bank_J, scene->bank_index.data(), scene->bank_weight.data(), on),
                                               "group_scene_fir_set_bank_at");
                                    else gcheck(g, pbso_group_scene_fir_set_at(g, t, h, on), "group_scene_fir_set_at");
                                },
                                [&](int64_t t, const float *dl) { gcheck(g, pbso_group_scene_fir_set_delay_at(g, t, dl), "group_scene_fir_set_delay_at"); });
        const std::vector<int> cuts = retune.cut(scene->cuts(n_buffers), n_buffers);
        for (size_t k = 0; k + 1 < cuts.size(); ++k) {
            retune.apply_at(cuts[k], group_set);
            if (scene->fir_schedule) {
                // (scheduled up front)
            } else if (scene->fir) {
                if (scene->fir_set_at(cuts[k], taps, onset)) {
                    if (scene->fir_bank)
                        gcheck(g, pbso_group_scene_fir_set_bank(g, scene->bank_J, scene->bank_index.data(), scene->bank_weight.data(), onset.data()),
                               "group_scene_fir_set_bank");
                    else gcheck(g, pbso_group_scene_fir_set(g, taps.data(), onset.data()), "group_scene_fir_set");
                }
                if (scene->fir_delay_set_at(cuts[k], fir_delay)) gcheck(g, pbso_group_scene_fir_set_delay(g, fir_delay.data()), "group_scene_fir_set_delay");
            } else if (scene->pan_schedule) {
                // (scheduled up front)
            } else if (scene->set_at(cuts[k], gain, delay)) gcheck(g, pbso_group_scene_mix_set(g, gain.data(), delay.data()), "group_scene_mix_set");
            const int nb = cuts[k + 1] - cuts[k];
            const size_t row = (size_t)nb * PBSO_FRAMES_PER_BUFFER;
            feed_ranks(cuts[k], cuts[k + 1]);
            gcheck(g, pbso_group_step(g, nb), "group_step");
            gcheck(g, pbso_group_gather(g, scene->fir ? PBSO_GATHER_FIR : PBSO_GATHER_SCENE), "group_gather");
            seg.resize((size_t)C * row);
            gcheck(g, pbso_group_read_result(g, 0, seg.data(), seg.size()), "group_read_result");
            for (int c = 0; c < C; ++c)
                std::copy(seg.begin() + (size_t)c * row, seg.begin() + (size_t)(c + 1) * row,
                          sound.begin() + (size_t)c * total + (size_t)cuts[k] * PBSO_FRAMES_PER_BUFFER);
        }
    } else {
        // (one step; with --retune the segments between its change points, each gathered as the on-device mix)
        sound.resize((size_t)n_buffers * PBSO_FRAMES_PER_BUFFER);
        const std::vector<int> cuts = retune.cut({0, n_buffers}, n_buffers);
        for (size_t k = 0; k + 1 < cuts.size(); ++k) {
            retune.apply_at(cuts[k], group_set);
            feed_ranks(cuts[k], cuts[k + 1]);
            gcheck(g, pbso_group_step(g, cuts[k + 1] - cuts[k]), "group_step");
            gcheck(g, pbso_group_gather(g, PBSO_GATHER_MIX), "group_gather");
            gcheck(g, pbso_group_read_result(g, 0, sound.data() + (size_t)cuts[k] * PBSO_FRAMES_PER_BUFFER,
                                             (size_t)(cuts[k + 1] - cuts[k]) * PBSO_FRAMES_PER_BUFFER), "group_read_result");
        }
    }
    std::printf("%d copies x %d audible modes on %d device(s): ranks own", copies, n_aud, (int)devices.size());
    for (int r = 0; r < (int)devices.size(); ++r) {
        int lo = 0, hi = 0;
        pbso_group_rank_span(g, r, &lo, &hi);
        std::printf(" [%d, %d)", lo, hi);
    }
    std::printf("\n");
    pbso_group_destroy(g);
    return 0;
}

// --eq: the script's lines; the coefficients in force, [S][5], are those of every channel
struct EqScript {
    struct Line { long b; int section, kind; double f0, q, gain; };
    std::vector<Line> lines;
    int S = 0, xfade = 441;
    bool schedule = false;                               // --eq-schedule: the lines are scheduled up front and cut nothing
    bool on() const { return S > 0; }
    void read(const std::string &path, int n_buffers) {
        static const char *kinds[] = {"lowpass", "highpass", "peak", "lowshelf", "highshelf"};
        std::ifstream f(path);
        if (!f) die("cannot read " + path);
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::istringstream iss(line);
            Line p;
            std::string kind;
            if (!(iss >> p.b >> p.section >> kind >> p.f0 >> p.q >> p.gain)) die("bad eq line (<buffer> <section> <kind> <f0> <Q> <gain dB>): " + line);
            p.kind = -1;
            for (int k = 0; k < 5; ++k)
                if (kind == kinds[k]) p.kind = k;
            if (p.kind < 0) die("eq kind must be lowpass, highpass, peak, lowshelf or highshelf: " + line);
            if (p.b < 0 || p.b >= n_buffers) die("eq line outside buffers 0 .. --buffers - 1: " + line);
            if (p.section < 0 || p.section >= pbso::EQ_MAX_SECTIONS) die("eq section must be 0 .. 7: " + line);
            if (const char *why = pbso::eq_design_refusal(p.kind, (double)PBSO_SAMPLE_RATE, p.f0, p.q, p.gain)) die(std::string("eq line: ") + why + ": " + line);
            S = std::max(S, p.section + 1);
            lines.push_back(p);
        }
        if (lines.empty()) die("no lines in " + path);
    }
    // --eq-schedule: the buffers that have lines, ascending
    std::vector<long> buffers() const {
        std::vector<long> b;
        for (const Line &p : lines) b.push_back(p.b);
        std::sort(b.begin(), b.end());
        b.erase(std::unique(b.begin(), b.end()), b.end());
        return b;
    }
    // ... and the schedule's rule on them (pbso_eq_set_at): the identity is a predecessor at sample 0
    void check_spacing() const {
        long long t_prev = 0;
        for (long b : buffers()) {
            const long long t = (long long)b * PBSO_FRAMES_PER_BUFFER;
            if (!pbso::eq_spacing_ok(t, t_prev, xfade))
                die("--eq-schedule: the lines of buffer " + std::to_string(b) + " are closer to their predecessor than the fade allows (--eq-xfade " +
                    std::to_string(xfade) + ": a set needs t_set - t_prev + 1 >= N, the first one against sample 0)");
            t_prev = t;
        }
    }
    std::vector<int> cut(std::vector<int> cuts, int n_buffers) const {
        for (const Line &p : lines)
            if (!schedule && p.b > 0 && p.b < n_buffers) cuts.push_back((int)p.b);
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        return cuts;
    }
    // the lines of buffer b into sos [S][5]; false when it has none
    bool set_at(long b, std::vector<double> &sos) const {
        bool any = false;
        for (const Line &p : lines)
            if (p.b == b) {
                if (pbso_eq_design(p.kind, (double)PBSO_SAMPLE_RATE, p.f0, p.q, p.gain, sos.data() + 5 * (size_t)p.section) != PBSO_OK) die("eq_design");
                any = true;
            }
        return any;
    }
};

int main(int argc, char **argv) {
    std::string d, name, mesh, modes, material, ffat, hits, track_hits, listener, out = "out.wav", raw, devices_arg, pan, fir, fir_dirs, fir_bank, fir_delay, reverb, strokes_file, arprm_arg, retune_arg, eq_arg, loudness_arg;
    double loudness_target = -23.0;
    bool loudness_flag = false;                          // --loudness-target was given
    EqScript eq;
    bool eq_flag = false;                                // --eq-xfade was given
    StrokeScript strokes;
    int n_buffers = 86, copies = 0, copy_shift = 1, time_chunks = 0;
    Scene scene;
    bool limit = false, pcm16 = false, master_flag = false;  // --limit; master_flag: one of its companions was given
    float limit_T = 1.f, master_gain = 1.f;
    int lookahead = 64, hold = 0;
    int out_rate = 0, rs_taps = 32;                      // --out-rate; rs_flag: one of its companions was given
    double rs_beta = 9.0, rs_cutoff = 0.9;
    bool rs_flag = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string { if (i + 1 >= argc) die("missing value for " + a); return argv[++i]; };
        if (a == "-d" || a == "--data_dir") d = val();
        else if (a == "-name" || a == "--obj_name") name = val();
        else if (a == "-m" || a == "--mesh") mesh = val();
        else if (a == "-s" || a == "--surf_mode") modes = val();
        else if (a == "-t" || a == "--material") material = val();
        else if (a == "-p" || a == "--ffat_map") ffat = val();
        else if (a == "--hits") hits = val();
        else if (a == "--track-hits") track_hits = val();
        else if (a == "--listener") listener = val();
        else if (a == "--strokes") strokes_file = val();
        else if (a == "--stroke-force") {
            const std::string t = val();
            if (t == "point") strokes.force_type = PBSO_POINT_FORCE;
            else if (t == "ar") strokes.force_type = PBSO_AUTOREGRESSIVE_FORCE;
            else die("--stroke-force must be point or ar");
        }
        else if (a == "--arprm") arprm_arg = val();
        else if (a == "--buffers") n_buffers = std::atoi(val().c_str());
        else if (a == "--out") out = val();
        else if (a == "--raw") raw = val();
        else if (a == "--devices") devices_arg = val();
        else if (a == "--copies") copies = std::atoi(val().c_str());
        else if (a == "--copy-shift") copy_shift = std::atoi(val().c_str());
        else if (a == "--channels") scene.channels = std::atoi(val().c_str());
        else if (a == "--pan") pan = val();
        else if (a == "--pan-schedule") scene.pan_schedule = true;
        else if (a == "--fir-schedule") scene.fir_schedule = true;
        else if (a == "--time-chunks") time_chunks = std::atoi(val().c_str());
        else if (a == "--retune") retune_arg = val();
        else if (a == "--ramp") scene.ramp = std::atoi(val().c_str());
        else if (a == "--fir") fir = val();
        else if (a == "--fir-dirs") fir_dirs = val();
        else if (a == "--fir-bank") fir_bank = val();
        else if (a == "--fir-taps") scene.n_taps = std::atoi(val().c_str());
        else if (a == "--fir-delay") fir_delay = val();
        else if (a == "--xfade") scene.xfade = std::atoi(val().c_str());
        else if (a == "--delay-ramp") scene.fir_delay_ramp = std::atoi(val().c_str());
        else if (a == "--reverb") reverb = val();
        else if (a == "--reverb-xfade") scene.reverb_xfade = std::atoi(val().c_str());
        else if (a == "--limit") { limit = true; limit_T = (float)std::atof(val().c_str()); }
        else if (a == "--lookahead") { master_flag = true; lookahead = std::atoi(val().c_str()); }
        else if (a == "--hold") { master_flag = true; hold = std::atoi(val().c_str()); }
        else if (a == "--gain") { master_flag = true; master_gain = (float)std::atof(val().c_str()); }
        else if (a == "--pcm16") pcm16 = true;
        else if (a == "--out-rate") { out_rate = std::atoi(val().c_str()); if (out_rate < 1) die("--out-rate: the rates must be positive"); }
        else if (a == "--rs-taps") { rs_flag = true; rs_taps = std::atoi(val().c_str()); }
        else if (a == "--rs-beta") { rs_flag = true; rs_beta = std::atof(val().c_str()); }
        else if (a == "--rs-cutoff") { rs_flag = true; rs_cutoff = std::atof(val().c_str()); }
        else if (a == "--eq") eq_arg = val();
        else if (a == "--eq-xfade") { eq_flag = true; eq.xfade = std::atoi(val().c_str()); }
        else if (a == "--eq-schedule") eq.schedule = true;
        else if (a == "--loudness") loudness_arg = val();
        else if (a == "--loudness-target") { loudness_flag = true; loudness_target = std::atof(val().c_str()); }
        else die("unknown flag " + a);
    }
    if (eq_flag && eq_arg.empty()) die("--eq-xfade belongs to --eq FILE");
    if (eq.schedule && eq_arg.empty()) die("--eq-schedule needs --eq FILE: it schedules that script's lines");
    if (!eq_arg.empty()) {
        if (!devices_arg.empty()) die("--eq runs on one engine, not through a device group (--devices)");
        if (!raw.empty()) die("--raw dumps the unscaled mix: not with --eq");
        if (scene.channels < 1 || scene.channels > 8 || (pan.empty() && fir.empty() && fir_dirs.empty()))
            die("--eq needs --channels C (1 .. 8) and one of --pan FILE or --fir FILE: it filters that mix");
        if (eq.xfade < 0 || eq.xfade > (1 << 20)) die("--eq-xfade must be 0 .. 1048576");
        eq.read(eq_arg, n_buffers);
        if (eq.schedule) eq.check_spacing();
    }
    if (loudness_flag && loudness_arg.empty()) die("--loudness-target belongs to --loudness FILE");
    if (!loudness_arg.empty()) {
        if (!devices_arg.empty()) die("--loudness runs on one engine, not through a device group (--devices)");
        if (!raw.empty()) die("--raw dumps the unscaled mix: not with --loudness");
        if (limit) die("--loudness measures in front of the limiter: not with --limit (measure, then render again with --limit T --gain G)");
        if (out_rate) die("--loudness measures at the engine's rate: not with --out-rate");
        if (!(std::isfinite(loudness_target) && loudness_target >= -70.0 && loudness_target <= 0.0)) die("--loudness-target must be -70 .. 0 LUFS");
    }
    const bool loud = !loudness_arg.empty();
    if (pcm16 && !limit) die("--pcm16 needs --limit T: an integer WAV clips without a ceiling");
    if (master_flag && !limit) die("--lookahead, --hold and --gain belong to --limit T");
    if (limit) {
        if (!devices_arg.empty()) die("--limit runs on one engine, not through a device group (--devices)");
        if (!raw.empty()) die("--raw dumps the unscaled mix: not with --limit");
        if (!(std::isfinite(limit_T) && limit_T > 0.f && limit_T <= 1.f)) die("--limit must be a ceiling in (0, 1]");
        if (lookahead < 1 || lookahead > 4096) die("--lookahead must be 1 .. 4096");
        if (hold < 0 || hold > 65536) die("--hold must be 0 .. 65536");
        if (!std::isfinite(master_gain)) die("--gain must be finite");
    }
    if (rs_flag && !out_rate) die("--rs-taps, --rs-beta and --rs-cutoff belong to --out-rate R");
    int rs_L = 1, rs_M = 1;
    if (out_rate) {
        if (!devices_arg.empty()) die("--out-rate runs on one engine, not through a device group (--devices)");
        if (!raw.empty()) die("--raw dumps the unscaled mix at 44100 Hz: not with --out-rate");
        if (const char *why = pbso::resample_refusal(PBSO_SAMPLE_RATE, out_rate, rs_taps, rs_beta, rs_cutoff))
            die(std::string("--out-rate from 44100 (L = R / gcd, M = 44100 / gcd): ") + why);
        pbso::resample_reduce(PBSO_SAMPLE_RATE, out_rate, rs_L, rs_M);
    }
    if (!d.empty()) {                                   // fixed directory structure, tools/...:480-495
        if (name.empty()) name = guess_name(d);
        std::printf("object name: %s\n", name.c_str());
        mesh = d + "/" + name + ".tet.obj";
        modes = d + "/" + name + "_surf.modes";
        material = d + "/" + name + "_material.txt";
        ffat = d + "/" + name + "_ffat_maps";
    }
    if (modes.empty() || material.empty()) die("need -d <dir> or -s <modes> -t <material> [-m <obj>] [-p <ffat dir>]");

    // assert(modes->numDOF() == V.rows()*3), tools/...:515
    int n_dof = 0, n_modes = 0;
    {
        double *om = nullptr, *md = nullptr;
        const int mrc = pbso_modes_read(modes.c_str(), &n_dof, &n_modes, &om, &md);
        if (mrc != PBSO_OK) die(std::string("modes_read: ") + pbso_status_string(mrc) + ": " + modes);
        pbso_free(om);
        pbso_free(md);
    }
    // igl::read_triangle_mesh(obj_file, V, F); igl::per_vertex_normals(V, F, VN);   tools/...:508-509
    std::vector<double> VN;
    if (!mesh.empty()) {
        int nv = 0, nf = 0;
        double *V = nullptr, *vn = nullptr;
        int *F = nullptr;
        const int orc = pbso_obj_read(mesh.c_str(), &nv, &nf, &V, &F, &vn);
        if (orc == PBSO_OK) {
            if (nv * 3 != n_dof) die("DOFs mismatch: .obj has " + std::to_string(nv) + " vertices, modes have nDOF " + std::to_string(n_dof));
            VN.assign(vn, vn + 3 * (size_t)nv);
            std::printf("mesh: %d vertices, %d triangles\n", nv, nf);
            pbso_free(V);
            pbso_free(F);
            pbso_free(vn);
        } else if (d.empty()) {
            die("cannot read mesh " + mesh);
        }
    }
    // the scripts that stand in for the camera and the mouse
    std::vector<Pos> path;
    if (!listener.empty()) {
        std::ifstream f(listener);
        if (!f) die("cannot read " + listener);
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::istringstream iss(line);
            Pos p;
            if (!(iss >> p.b >> p.p[0] >> p.p[1] >> p.p[2])) die("bad listener line: " + line);
            path.push_back(p);
        }
    }
    std::vector<Hit> hit_list;
    if (!hits.empty()) {
        std::ifstream f(hits);
        if (!f) die("cannot read " + hits);
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::istringstream iss(line);
            long b; int vid; double n[3]; std::string type = "point", tok;
            if (!(iss >> b >> vid >> tok)) die("bad hit line: " + line);
            if (tok == "-") {                                // the tool's own path: vn = VN.row(vid), tools/...:607
                if (VN.empty()) die("hit without a normal needs the mesh (-m / -d)");
                if (vid < 0 || 3 * (size_t)vid + 2 >= VN.size()) die("vertex id out of range: " + line);
                for (int j = 0; j < 3; ++j) n[j] = VN[3 * (size_t)vid + j];
            } else {
                n[0] = std::atof(tok.c_str());
                if (!(iss >> n[1] >> n[2])) die("bad hit line: " + line);
            }
            iss >> type;
            Hit h;
            h.b = b;
            std::memset(&h.m, 0, sizeof(h.m));
            h.m.data_kind = PBSO_DATA_VERTEX;
            h.m.vids[0] = vid;
            const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);   // VN.row(vid).normalized(), tools/...:607
            for (int j = 0; j < 3; ++j) h.m.vn[j] = n[j] / len;
            if (type == "gauss") { h.m.force_type = PBSO_GAUSSIAN_FORCE; iss >> h.m.gaussian_width_us; }
            else if (type == "ar") h.m.force_type = PBSO_AUTOREGRESSIVE_FORCE;
            else h.m.force_type = PBSO_POINT_FORCE;
            hit_list.push_back(h);
        }
    }
    std::vector<std::vector<float>> tracks;
    if (!track_hits.empty()) {
        std::ifstream f(track_hits);
        if (!f) die("cannot read " + track_hits);
        std::vector<std::string> paths;
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::istringstream iss(line);
            long b; int start, vid; double n[3]; std::string tok, file;
            if (!(iss >> b >> start >> vid >> tok)) die("bad track-hit line: " + line);
            if (tok == "-") {
                if (VN.empty()) die("hit without a normal needs the mesh (-m / -d)");
                if (vid < 0 || 3 * (size_t)vid + 2 >= VN.size()) die("vertex id out of range: " + line);
                for (int j = 0; j < 3; ++j) n[j] = VN[3 * (size_t)vid + j];
            } else {
                n[0] = std::atof(tok.c_str());
                if (!(iss >> n[1] >> n[2])) die("bad track-hit line: " + line);
            }
            if (!(iss >> file)) die("bad track-hit line (track file): " + line);
            Hit h;
            h.b = b;
            std::memset(&h.m, 0, sizeof(h.m));
            std::memset(&h.play, 0, sizeof(h.play));
            h.m.force_type = PBSO_TRACK_FORCE;
            h.m.data_kind = PBSO_DATA_VERTEX;
            h.m.vids[0] = vid;
            const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            for (int j = 0; j < 3; ++j) h.m.vn[j] = n[j] / len;
            h.play.start_sample = start;
            h.play.gain = 1.0; h.play.rate = 1.0;
            long long ns = 0; int loop = 0;
            if (iss >> h.play.gain && iss >> h.play.rate && iss >> h.play.first && iss >> ns && iss >> loop) {}
            h.play.n_samples = ns;
            h.play.loop = loop;
            auto at = std::find(paths.begin(), paths.end(), file);
            h.track = (int)(at - paths.begin());
            if (at == paths.end()) { paths.push_back(file); tracks.push_back(read_track_file(file)); }
            hit_list.push_back(h);
        }
        // one queue: in buffer order, the --hits line first at equal buffers (a message cannot overtake an earlier one)
        std::stable_sort(hit_list.begin(), hit_list.end(), [](const Hit &a, const Hit &b) { return a.b < b.b; });
    }

    if (!strokes_file.empty()) {
        std::ifstream f(strokes_file);
        if (!f) die("cannot read " + strokes_file);
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::istringstream iss(line);
            Stroke s;
            std::memset(&s, 0, sizeof(s));
            std::string tok, flag;
            if (!(iss >> s.b >> tok)) die("bad stroke line: " + line);
            if (tok == "-") {
                s.flags = PBSO_STROKE_ZERO;
            } else {
                s.v[0] = std::atoi(tok.c_str());
                if (!(iss >> s.v[1] >> s.v[2] >> s.c[0] >> s.c[1] >> s.c[2] >> s.n[0] >> s.n[1] >> s.n[2])) die("bad stroke line: " + line);
                for (int j = 0; j < 3; ++j)
                    if (s.v[j] < 0 || 3 * s.v[j] + 2 >= n_dof) die("vertex id out of range: " + line);
            }
            if (iss >> flag) {
                if (flag == "start") s.flags |= PBSO_STROKE_START;
                else if (flag == "end") s.flags |= PBSO_STROKE_END;
                else die("bad stroke line (start or end): " + line);
            }
            if (s.b < 0) die("bad stroke line: " + line);
            strokes.entries.push_back(s);
        }
        std::stable_sort(strokes.entries.begin(), strokes.entries.end(), [](const Stroke &a, const Stroke &b) { return a.b < b.b; });
    }
    if (!arprm_arg.empty()) {
        std::istringstream iss(arprm_arg);
        if (!(iss >> strokes.arprm[0] >> strokes.arprm[1] >> strokes.arprm[2] >> strokes.arprm[3])) die("--arprm needs \"<a0> <a1> <sigma> <mu>\"");
        strokes.have_arprm = true;
    }
    std::vector<int> devices;
    if (!devices_arg.empty()) {
        std::istringstream ds(devices_arg);
        std::string tok;
        while (std::getline(ds, tok, ',')) devices.push_back(std::atoi(tok.c_str()));
        if (devices.empty()) die("--devices needs a list of HIP ordinals");
        if (copies <= 0) copies = (int)devices.size();
    }
    RetuneScript retune;
    if (!retune_arg.empty()) retune.read(retune_arg, devices.empty() ? 1 : copies, n_buffers);
    // --fir-dirs is --fir with another kind of line: everything below that asks for --fir is answered by it
    if (!fir_dirs.empty() && (!fir.empty() || !pan.empty())) die("--fir-dirs excludes --fir and --pan: one script sets the filters");
    if (fir_dirs.empty() != fir_bank.empty()) die("--fir-bank FILE --fir-taps K and --fir-dirs SCRIPT go together");
    if (fir_dirs.empty() && scene.n_taps != 0) die("--fir-taps belongs to --fir-bank: taps files tell their own length");
    if (!fir_dirs.empty()) {
        fir = fir_dirs;
        scene.fir_bank = true;
    }
    const bool mixed = scene.channels != 0 || !pan.empty() || !fir.empty();
    if (!pan.empty() && !fir.empty()) die("--pan and --fir exclude each other: one mixer writes the WAV");
    if (scene.pan_schedule && pan.empty()) die("--pan-schedule needs --pan FILE: it schedules that script's lines");
    if (scene.fir_schedule && fir.empty()) die("--fir-schedule needs --fir FILE: it schedules that script's lines (and --fir-delay's)");
    if (!fir_delay.empty() && fir.empty()) die("--fir-delay needs --fir FILE: the delay sits in front of the filter mix");
    if (mixed && (scene.channels < 1 || scene.channels > 8)) die("--channels must be 1 .. 8");
    if (!fir.empty()) {
        // the scene filter mix's script: <buffer> <copy> <onset> <taps file>
        if (scene.xfade < 0 || scene.xfade > (1 << 20)) die("--xfade must be 0 .. 1048576");
        scene.fir = true;
        scene.copies = devices.empty() ? 1 : copies;
        if (scene.fir_bank) {
            // the bank: raw little-endian f32 [F][--channels][--fir-taps]; F follows from the file's size
            if (scene.n_taps < 1 || scene.n_taps > 1024) die("--fir-taps must be 1 .. 1024");
            std::ifstream bf(fir_bank, std::ios::binary);
            if (!bf) die("cannot read bank file " + fir_bank);
            const std::string bytes((std::istreambuf_iterator<char>(bf)), std::istreambuf_iterator<char>());
            const size_t per = (size_t)scene.channels * scene.n_taps * 4;
            if (bytes.empty() || bytes.size() % per != 0 || bytes.size() / per > ((size_t)1 << 20))
                die("bank file " + fir_bank + " is not float32 [F][--channels][--fir-taps] with F 1 .. 1048576 (" + std::to_string(bytes.size()) + " bytes)");
            scene.bank_F = (int)(bytes.size() / per);
            scene.bank.resize(bytes.size() / 4);
            std::memcpy(scene.bank.data(), bytes.data(), bytes.size());
        }
        std::ifstream f(fir);
        if (!f) die("cannot read " + fir);
        std::vector<std::string> paths;
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::istringstream iss(line);
            FirLine p;
            std::string path;
            if (scene.fir_bank) {
                // --fir-dirs: <buffer> <copy> <onset> <i0> <w0> [<i1> <w1> ... up to 8 pairs]
                if (!(iss >> p.b >> p.copy >> p.onset)) die("bad fir-dirs line (<buffer> <copy> <onset> <index> <weight> ...): " + line);
                // (every token is parsed whole: "0.5" where an index belongs is refused, not read as index 0 and weight .5)
                std::string ti, tw;
                while (iss >> ti) {
                    if (!(iss >> tw)) die("fir-dirs line with an index that has no weight: " + line);
                    char *end = nullptr;
                    const long ix = std::strtol(ti.c_str(), &end, 10);
                    if (end == ti.c_str() || *end != '\0') die("fir-dirs index is not an integer (pairs of <index> <weight>): " + line);
                    const float w = std::strtof(tw.c_str(), &end);
                    if (end == tw.c_str() || *end != '\0') die("fir-dirs weight is not a number (pairs of <index> <weight>): " + line);
                    if (ix < 0 || ix >= scene.bank_F) die("fir-dirs index outside the bank's 0 .. " + std::to_string(scene.bank_F - 1) + ": " + line);
                    if (!std::isfinite(w)) die("fir-dirs weight is not finite: " + line);
                    p.pairs.push_back({(int)ix, w});
                }
                if (p.pairs.empty() || p.pairs.size() > 8) die("fir-dirs line needs 1 .. 8 pairs of <index> <weight>: " + line);
                scene.bank_J = std::max(scene.bank_J, (int)p.pairs.size());
            } else if (!(iss >> p.b >> p.copy >> p.onset >> path)) die("bad fir line (<buffer> <copy> <onset> <taps file>): " + line);
            if (p.copy < 0 || p.copy >= scene.copies) die("fir line for a copy that does not exist: " + line);
            if (p.b < 0 || p.b >= n_buffers) die("fir line outside buffers 0 .. --buffers - 1: " + line);
            if (p.onset < 0 || p.onset > (1 << 20)) die("fir onset outside [0, 1048576]: " + line);
            p.file = scene.fir_bank ? -1 : (int)(std::find(paths.begin(), paths.end(), path) - paths.begin());
            if (!scene.fir_bank && p.file == (int)paths.size()) {   // a path not seen yet: loaded once
                paths.push_back(path);
                std::ifstream tf(path, std::ios::binary);
                if (!tf) die("cannot read taps file " + path);
                const std::string bytes((std::istreambuf_iterator<char>(tf)), std::istreambuf_iterator<char>());
                const size_t per = (size_t)scene.channels * 4;
                if (bytes.empty() || bytes.size() % per != 0 || bytes.size() / per > 1024)
                    die("taps file " + path + " is not float32 [--channels][K] with K 1 .. 1024 (" + std::to_string(bytes.size()) + " bytes)");
                const int K = (int)(bytes.size() / per);
                if (scene.n_taps != 0 && K != scene.n_taps)
                    die("taps file " + path + " holds " + std::to_string(K) + " taps per channel, the files before it " + std::to_string(scene.n_taps));
                scene.n_taps = K;
                std::vector<float> h((size_t)scene.channels * K);
                std::memcpy(h.data(), bytes.data(), bytes.size());
                scene.fir_files.push_back(h);
            }
            scene.max_onset = std::max(scene.max_onset, p.onset);
            scene.fir_lines.push_back(p);
        }
        if (scene.fir_lines.empty()) die("no lines in " + fir);
        scene.bank_index.assign((size_t)scene.copies * scene.bank_J, 0);
        scene.bank_weight.assign((size_t)scene.copies * scene.bank_J, 0.f);
        if (!fir_delay.empty()) {
            // the delay stage's script: <buffer> <copy> <delay in samples>; max_delay is the largest value, rounded up
            if (scene.fir_delay_ramp < 0 || scene.fir_delay_ramp > (1 << 20)) die("--delay-ramp must be 0 .. 1048576");
            std::ifstream df(fir_delay);
            if (!df) die("cannot read " + fir_delay);
            while (std::getline(df, line)) {
                if (line.empty() || line[0] == '#') continue;
                std::istringstream iss(line);
                FirDelayLine p;
                if (!(iss >> p.b >> p.copy >> p.delay)) die("bad fir-delay line (<buffer> <copy> <delay in samples>): " + line);
                if (p.copy < 0 || p.copy >= scene.copies) die("fir-delay line for a copy that does not exist: " + line);
                if (p.b < 0 || p.b >= n_buffers) die("fir-delay line outside buffers 0 .. --buffers - 1: " + line);
                if (!(p.delay >= 0.f && p.delay <= (float)(1 << 20))) die("fir delay outside [0, 1048576]: " + line);
                scene.fir_max_delay = std::max(scene.fir_max_delay, (int)std::ceil(p.delay));
                scene.fir_delay_lines.push_back(p);
            }
            if (scene.fir_delay_lines.empty()) die("no lines in " + fir_delay);
        }
    } else if (mixed) {
        // the scene mix's script: <buffer> <copy> then a gain and a delay per channel
        if (pan.empty()) die("--channels needs --pan FILE or --fir FILE");
        if (scene.ramp < 0 || scene.ramp > (1 << 20)) die("--ramp must be 0 .. 1048576");
        scene.copies = devices.empty() ? 1 : copies;
        std::ifstream f(pan);
        if (!f) die("cannot read " + pan);
        std::string line;
        double dmax = 0;
        while (std::getline(f, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::istringstream iss(line);
            Pan p;
            if (!(iss >> p.b >> p.copy)) die("bad pan line: " + line);
            p.gd.resize(2 * (size_t)scene.channels);
            for (float &v : p.gd)
                if (!(iss >> v)) die("bad pan line (a gain and a delay per channel): " + line);
            if (p.copy < 0 || p.copy >= scene.copies) die("pan line for a copy that does not exist: " + line);
            if (p.b < 0 || p.b >= n_buffers) die("pan line outside buffers 0 .. --buffers - 1: " + line);
            for (int c = 0; c < scene.channels; ++c)
                if (!(p.gd[2 * c + 1] >= 0.f && p.gd[2 * c + 1] <= (float)(1 << 20))) die("pan delay outside [0, 1048576]: " + line);
            for (int c = 0; c < scene.channels; ++c) dmax = std::max(dmax, (double)p.gd[2 * c + 1]);
            scene.lines.push_back(p);
        }
        scene.max_delay = (int)std::ceil(dmax);
    }
    if (!reverb.empty()) {
        if (scene.channels == 0 || (pan.empty() && fir.empty())) die("--reverb needs --channels C and one of --pan FILE or --fir FILE: the wet signal is added to that mix");
        if (!devices.empty()) die("--reverb runs on one engine, not through a device group (--devices)");
        if (scene.reverb_xfade < 0 || scene.reverb_xfade > (1 << 20)) die("--reverb-xfade must be 0 .. 1048576");
        std::ifstream rf(reverb, std::ios::binary);
        if (!rf) die("cannot read impulse response " + reverb);
        const std::string bytes((std::istreambuf_iterator<char>(rf)), std::istreambuf_iterator<char>());
        const size_t per = (size_t)scene.channels * 4;
        if (bytes.empty() || bytes.size() % per != 0 || bytes.size() / per > (size_t)(1 << 17))
            die("impulse response " + reverb + " is not float32 [--channels][K] with K 1 .. 131072 (" + std::to_string(bytes.size()) + " bytes)");
        scene.reverb_taps = (int)(bytes.size() / per);
        scene.reverb.resize((size_t)scene.channels * scene.reverb_taps);
        std::memcpy(scene.reverb.data(), bytes.data(), bytes.size());
    }
    std::vector<float> sound((size_t)n_buffers * PBSO_FRAMES_PER_BUFFER);
    std::vector<int16_t> pcm;                            // --pcm16: the master bus's (the resampler's) frames, interleaved, segment behind segment
    std::vector<std::vector<float>> resampled;           // --out-rate: the resampler's output per channel, segment behind segment
    // --out-rate: the delay in front of the file is d = look-ahead + (L T - 1) / (2 L) input samples = rs_delay_num / (2 L); the
    // output frames dropped for it, floor(d L / M + 0.5), and the frames written, ceil(buffers * 513 * L / M)
    const long long rs_delay_num = out_rate ? 2LL * rs_L * (limit ? lookahead : 0) + ((long long)rs_L * rs_taps - 1) : 0;
    const long long rs_drop = out_rate ? (rs_delay_num + rs_M) / (2LL * rs_M) : 0;
    const long long rs_keep = out_rate ? pbso::resample_max_out((long long)n_buffers * PBSO_FRAMES_PER_BUFFER, rs_L, rs_M) : 0;
    double device_ms = 0;
    if (!devices.empty()) {
        run_group(devices, copies, copy_shift, modes, material, ffat, hit_list, tracks, path, strokes, n_buffers, mixed ? &scene : nullptr, retune, time_chunks, sound);
    } else {
        pbso_engine_desc desc;
        std::memset(&desc, 0, sizeof(desc));
        desc.abi_version = PBSO_ABI_VERSION;
        desc.qnorm_mode = PBSO_QNORM_OFF;
        desc.time_chunks = time_chunks;
        pbso_engine *e = nullptr;
        int rc = pbso_engine_create(&desc, &e);
        check(e, rc, "engine_create");
        int obj = -1, n_aud = 0;
        check(e, pbso_add_object_from_files(e, modes.c_str(), material.c_str(), ffat.empty() ? nullptr : ffat.c_str(), &obj, &n_aud),
              "add_object_from_files");
        std::printf("modes: %d of %d audible, nDOF %d\n", n_aud, n_modes, n_dof);
        check(e, pbso_finalize(e), "finalize");
        for (const Pos &p : path) check(e, pbso_compute_transfer(e, obj, p.p, p.b), "compute_transfer");
        if (path.empty()) check(e, pbso_set_use_transfer(e, obj, 0, 0), "set_use_transfer");   // unit transfer
        const std::vector<int> track_ids = create_tracks(e, tracks);
        for (const Hit &h : hit_list) {
            if ((limit || out_rate) && h.b >= n_buffers) continue;   // (the tail behind the run: no hits, as the run without --limit has none)
            rc = enqueue_hit(e, obj, h, track_ids, h.b);
            check(e, rc, h.track < 0 ? "enqueue_force" : "enqueue_track_force");
            if (rc == 0) die("force queue full");
        }
        if (strokes.have_arprm) check(e, pbso_enqueue_arprm(e, obj, strokes.arprm, strokes.arprm[2], strokes.arprm[3], 0), "enqueue_arprm");
        StrokeFeed feed;                                     // (borrowed by the engine until the step that follows returns)
        const std::vector<int> stroke_ids{obj};
        const std::vector<long> stroke_shift{0};
        // --limit: n_tail more buffers behind the scripts; every segment read back goes, scaled as the WAV would have been, through
        // the master bus, and what comes out replaces it in `sound` (PCM: in `pcm`, interleaved)
        const int channels_out = mixed ? scene.channels : 1;
        int n_tail = limit ? (lookahead + PBSO_FRAMES_PER_BUFFER - 1) / PBSO_FRAMES_PER_BUFFER : 0;
        if (out_rate) {
            // --out-rate: as many as hold d, and then as many as it takes until the outputs dropped and written are all there
            n_tail = (int)((rs_delay_num + 2LL * rs_L * PBSO_FRAMES_PER_BUFFER - 1) / (2LL * rs_L * PBSO_FRAMES_PER_BUFFER));
            while (pbso::resample_max_out((long long)(n_buffers + n_tail) * PBSO_FRAMES_PER_BUFFER, rs_L, rs_M) < rs_drop + rs_keep) ++n_tail;
        }
        const int n_run = n_buffers + n_tail;
        const bool post = limit || out_rate || eq.on() || loud;      // the segments go through a bus behind the mix
        void *m_in = nullptr;
        if (post && pbso_host_alloc((size_t)channels_out * n_run * PBSO_FRAMES_PER_BUFFER * sizeof(float), &m_in) != PBSO_OK)
            die("cannot allocate the master bus's input");
        if (limit) {
            check(e, pbso_master_enable(e, channels_out, limit_T, lookahead, hold, 0), "master_enable");
            check(e, pbso_master_set_gain(e, master_gain), "master_set_gain");
        }
        if (out_rate) {
            check(e, pbso_resample_enable(e, channels_out, out_rate, rs_taps, rs_beta, rs_cutoff), "resample_enable");
            resampled.resize(channels_out);
        }
        const int loud_hop = pbso::loudness_hop(PBSO_SAMPLE_RATE);
        if (loud)
            check(e, pbso_loudness_enable(e, channels_out, nullptr, (int)((long long)n_run * PBSO_FRAMES_PER_BUFFER / loud_hop) + 1, 1), "loudness_enable");
        std::vector<double> eq_sos;                          // --eq: [C][S][5], every channel alike
        if (eq.on()) {
            check(e, pbso_eq_enable(e, channels_out, eq.S, eq.xfade), "eq_enable");
            eq_sos.assign((size_t)channels_out * eq.S * 5, 0.0);
            for (size_t i = 0; i < eq_sos.size(); i += 5) eq_sos[i] = 1.0;
        }
        // --eq: the lines of buffer b, given to every channel, before the step that begins there
        auto eq_set_at = [&](int b) {
            std::vector<double> one(eq_sos.begin(), eq_sos.begin() + (size_t)eq.S * 5);
            if (!eq.on() || eq.schedule || !eq.set_at(b, one)) return;
            for (int c = 0; c < channels_out; ++c) std::copy(one.begin(), one.end(), eq_sos.begin() + (size_t)c * eq.S * 5);
            check(e, pbso_eq_set(e, eq_sos.data()), "eq_set");
        };
        // --eq-schedule: every buffer that has lines, in order, as one set at its first sample
        if (eq.on() && eq.schedule)
            for (long b : eq.buffers()) {
                std::vector<double> one(eq_sos.begin(), eq_sos.begin() + (size_t)eq.S * 5);
                eq.set_at(b, one);
                for (int c = 0; c < channels_out; ++c) std::copy(one.begin(), one.end(), eq_sos.begin() + (size_t)c * eq.S * 5);
                check(e, pbso_eq_set_at(e, (int64_t)b * PBSO_FRAMES_PER_BUFFER, eq_sos.data()), "eq_set_at");
            }
        auto master_segment = [&](std::vector<float> &seg) {         // seg [C][row], the last step's
            float *in = (float *)m_in;
            for (size_t i = 0; i < seg.size(); ++i) in[i] = (float)((double)seg[i] / 1E10);
            // --eq in place, in front of the limiter and the resampler
            if (eq.on()) check(e, pbso_eq(e, m_in, m_in), "eq");
            // --loudness behind it, on the samples of the WAV
            if (loud) check(e, pbso_loudness(e, m_in), "loudness");
            if (!limit && !out_rate) {
                if (eq.on()) check(e, pbso_read_eq(e, seg.data(), seg.size()), "read_eq");
                else check(e, pbso_sync(e), "sync");                 // (the next segment overwrites the bus's input; seg stays the unscaled mix)
                return;
            }
            if (out_rate) {
                // the limiter in place (its input is read before anything is written), the resampler behind it from the same buffer
                if (limit) check(e, pbso_master(e, m_in, m_in), "master");
                int64_t k = 0;
                check(e, pbso_resample(e, m_in, nullptr, 0, &k), "resample");
                if (pcm16) {
                    const size_t at = pcm.size();
                    pcm.resize(at + (size_t)k * channels_out);
                    check(e, pbso_read_resample_pcm16(e, pcm.data() + at, (size_t)k * channels_out), "read_resample_pcm16");
                } else {
                    std::vector<float> y((size_t)k * channels_out);
                    check(e, pbso_read_resample(e, y.data(), y.size()), "read_resample");
                    for (int c = 0; c < channels_out; ++c) resampled[c].insert(resampled[c].end(), y.begin() + (size_t)c * k, y.begin() + (size_t)(c + 1) * k);
                }
                return;
            }
            check(e, pbso_master(e, m_in, nullptr), "master");
            if (pcm16) {
                const size_t at = pcm.size();
                pcm.resize(at + seg.size());
                check(e, pbso_read_master_pcm16(e, pcm.data() + at, seg.size()), "read_master_pcm16");
            } else {
                check(e, pbso_read_master(e, seg.data(), seg.size()), "read_master");
            }
        };
        auto engine_set = [&](int n, const int *ids, const pbso_material *mats, int keep) {
            check(e, pbso_set_material(e, n, ids, mats, keep), "set_material");      // (one object: copy 0 is object 0)
        };
        if (mixed) {
            // the one object through the scene mixer, segment by segment: sound [C][n_buffers * B]
            const int C = scene.channels;
            const size_t total = (size_t)n_run * PBSO_FRAMES_PER_BUFFER;
            if (scene.fir) check(e, pbso_scene_fir_enable(e, C, scene.n_taps, scene.max_onset, scene.xfade), "scene_fir_enable");
            else check(e, pbso_scene_mix_enable(e, C, scene.max_delay, scene.ramp), "scene_mix_enable");
            if (scene.fir_bank) check(e, pbso_scene_fir_bank_create(e, scene.bank_F, scene.bank.data()), "scene_fir_bank_create");
            if (!scene.fir_delay_lines.empty())
                check(e, pbso_scene_fir_delay_enable(e, scene.fir_max_delay, scene.fir_delay_ramp), "scene_fir_delay_enable");
            std::vector<float> delay_now(1, 0.f);
            std::vector<float> gain(C, 0.f), delay(C, 0.f), seg;
            std::vector<float> taps(scene.fir ? (size_t)C * scene.n_taps : 0, 0.f);
            std::vector<int> onset(1, 0);
            sound.assign((size_t)C * total, 0.f);
            // --reverb: the mix goes to `dry` and the object mix to `bus`, device-visible memory both, instead of the engine's own
            // buffers; the reverb reads the bus, adds its result to the dry mix and is what is read back
            void *dry = nullptr, *bus = nullptr;
            if (scene.reverb_taps) {
                if (pbso_host_alloc((size_t)C * total * sizeof(float), &dry) != PBSO_OK || pbso_host_alloc(total * sizeof(float), &bus) != PBSO_OK)
                    die("cannot allocate the reverb's buffers");
                check(e, pbso_scene_reverb_enable(e, 1, C, scene.reverb_taps, scene.reverb_xfade), "scene_reverb_enable");
                check(e, pbso_scene_reverb_set(e, scene.reverb.data()), "scene_reverb_set");
            }
            if (scene.pan_schedule)
                scene.schedule_pan(gain, delay, [&](int64_t t, const float *gn, const float *dl) {
                    check(e, pbso_scene_mix_set_at(e, t, gn, dl), "scene_mix_set_at");
                });
            if (scene.fir_schedule)
                scene.schedule_fir(taps, onset, delay_now,
                                   [&](int64_t t, const float *h, const int *on) {
                                       if (scene.fir_bank)
                                           check(e, pbso_scene_fir_set_bank_at(e, t, scene.bank_J, scene.bank_index.data(), scene.bank_weight.data(), on),
                                                 "scene_fir_set_bank_at");
                                       else check(e, pbso_scene_fir_set_at(e, t, h, on), "scene_fir_set_at");
                                   },
                                   [&](int64_t t, const float *dl) { check(e, pbso_scene_fir_set_delay_at(e, t, dl), "scene_fir_set_delay_at"); });
            std::vector<int> cuts = eq.cut(retune.cut(scene.cuts(n_buffers), n_buffers), n_buffers);
            if (n_tail) cuts.push_back(n_run);
            for (size_t k = 0; k + 1 < cuts.size(); ++k) {
                if (cuts[k] < n_buffers) retune.apply_at(cuts[k], engine_set);
                if (cuts[k] < n_buffers) eq_set_at(cuts[k]);
                if (cuts[k] >= n_buffers) {
                    // (--limit's tail: the script ended with the run)
                } else if (scene.fir_schedule) {
                    // (scheduled up front)
                } else if (scene.fir) {
                    if (scene.fir_set_at(cuts[k], taps, onset)) {
                        if (scene.fir_bank)
                            check(e, pbso_scene_fir_set_bank(e, scene.bank_J, scene.bank_index.data(), scene.bank_weight.data(), onset.data()),
                                  "scene_fir_set_bank");
                        else check(e, pbso_scene_fir_set(e, taps.data(), onset.data()), "scene_fir_set");
                    }
                    if (scene.fir_delay_set_at(cuts[k], delay_now)) check(e, pbso_scene_fir_set_delay(e, delay_now.data()), "scene_fir_set_delay");
                } else if (scene.pan_schedule) {
                    // (scheduled up front)
                } else if (scene.set_at(cuts[k], gain, delay)) check(e, pbso_scene_mix_set(e, gain.data(), delay.data()), "scene_mix_set");
                const int nb = cuts[k + 1] - cuts[k];
                const size_t row = (size_t)nb * PBSO_FRAMES_PER_BUFFER;
                if (cuts[k] < n_buffers) feed_strokes(e, strokes, stroke_ids, stroke_shift, cuts[k], cuts[k + 1], feed);
                check(e, pbso_step(e, nb), "step");
                seg.resize((size_t)C * row);
                if (scene.fir) check(e, pbso_scene_fir(e, dry), "scene_fir");
                else check(e, pbso_scene_mix(e, dry), "scene_mix");
                if (scene.reverb_taps) {
                    check(e, pbso_mix_objects(e, bus), "mix_objects");
                    check(e, pbso_scene_reverb(e, bus, dry, nullptr), "scene_reverb");
                    check(e, pbso_read_scene_reverb(e, seg.data(), seg.size()), "read_scene_reverb");
                } else if (scene.fir) {
                    check(e, pbso_read_scene_fir(e, seg.data(), seg.size()), "read_scene_fir");
                } else {
                    check(e, pbso_read_scene_mix(e, seg.data(), seg.size()), "read_scene_mix");
                }
                if (post) master_segment(seg);
                for (int c = 0; c < C; ++c)
                    std::copy(seg.begin() + (size_t)c * row, seg.begin() + (size_t)(c + 1) * row,
                              sound.begin() + (size_t)c * total + (size_t)cuts[k] * PBSO_FRAMES_PER_BUFFER);
            }
            if (scene.reverb_taps) check(e, pbso_sync(e), "sync");
            pbso_host_free(dry);
            pbso_host_free(bus);
        } else {
            sound.resize((size_t)n_run * PBSO_FRAMES_PER_BUFFER);
            if (retune.empty()) {
                feed_strokes(e, strokes, stroke_ids, stroke_shift, 0, n_buffers, feed);
                check(e, pbso_step(e, n_run), "step");
                check(e, pbso_read_audio(e, sound.data(), sound.size()), "read_audio");
                if (post) master_segment(sound);
            } else {
                // the segments between the material script's change points (--limit's tail behind the last one)
                std::vector<int> cuts = retune.cut({0, n_buffers}, n_buffers);
                cuts.back() = n_run;
                std::vector<float> seg;
                for (size_t k = 0; k + 1 < cuts.size(); ++k) {
                    retune.apply_at(cuts[k], engine_set);
                    feed_strokes(e, strokes, stroke_ids, stroke_shift, cuts[k], std::min(cuts[k + 1], n_buffers), feed);
                    check(e, pbso_step(e, cuts[k + 1] - cuts[k]), "step");
                    seg.resize((size_t)(cuts[k + 1] - cuts[k]) * PBSO_FRAMES_PER_BUFFER);
                    check(e, pbso_read_audio(e, seg.data(), seg.size()), "read_audio");
                    if (post) master_segment(seg);
                    std::copy(seg.begin(), seg.end(), sound.begin() + (size_t)cuts[k] * PBSO_FRAMES_PER_BUFFER);
                }
            }
        }
        if (post) check(e, pbso_sync(e), "sync");
        if (loud) {
            pbso_loudness_summary r;
            check(e, pbso_loudness_report(e, &r), "loudness_report");
            std::vector<pbso_loudness_block> blocks((size_t)r.n_blocks * channels_out);
            check(e, pbso_read_loudness_blocks(e, 0, r.n_blocks, blocks.data()), "read_loudness_blocks");
            FILE *f = std::fopen(loudness_arg.c_str(), "w");
            if (!f) die("cannot write " + loudness_arg);
            const double values[8] = {r.integrated, r.momentary, r.short_term, r.max_momentary, r.max_short_term, r.relative_threshold, r.true_peak, r.sample_peak};
            const char *keys[8] = {"integrated", "momentary", "short_term", "max_momentary", "max_short_term", "relative_threshold", "true_peak", "sample_peak"};
            for (int k = 0; k < 8; ++k) std::fprintf(f, "%s %.17g\n", keys[k], values[k]);
            std::fprintf(f, "n_blocks %lld\nn_gated %lld\n", (long long)r.n_blocks, (long long)r.n_gated);
            std::fprintf(f, "target %.17g\ngain_to_target %.17g\n", loudness_target, std::pow(10.0, (loudness_target - r.integrated) / 20.0));
            for (long long j = 0; j < (long long)r.n_blocks; ++j)
                for (int c = 0; c < channels_out; ++c) {
                    const pbso_loudness_block &b = blocks[(size_t)j * channels_out + c];
                    std::fprintf(f, "energy.%lld.%d %.17g\ntrue_peak.%lld.%d %.17g\nsample_peak.%lld.%d %.17g\n", j, c, b.energy, j, c, (double)b.true_peak, j, c,
                                 (double)b.sample_peak);
                }
            std::fclose(f);
            std::printf("loudness: integrated %.2f LUFS, true peak %.2f dBTP, gain to %.1f LUFS %.4f -> %s\n", r.integrated,
                        20.0 * std::log10(r.true_peak), loudness_target, std::pow(10.0, (loudness_target - r.integrated) / 20.0), loudness_arg.c_str());
        }
        pbso_host_free(m_in);
        pbso_engine_info info;
        check(e, pbso_get_info(e, &info), "get_info");
        device_ms = mixed ? info.total_device_ms : info.last_step_device_ms;      // (the scene mix steps in segments)
        pbso_engine_destroy(e);
    }
    // C channels interleaved (mono: as it stands)
    const int channels = mixed ? scene.channels : 1;
    if (out_rate) {
        // the resampler's output is in the WAV's scale already; it is d L / M output frames late
        const size_t drop = (size_t)rs_drop, keep = (size_t)rs_keep;
        if (pcm16) {
            if (pcm.size() < (drop + keep) * channels) die("the resampler delivered fewer frames than the file holds");
            write_wav_pcm16(out, std::vector<int16_t>(pcm.begin() + drop * channels, pcm.begin() + (drop + keep) * channels), out_rate, channels);
        } else {
            if (resampled[0].size() < drop + keep) die("the resampler delivered fewer frames than the file holds");
            std::vector<float> wav(keep * channels);
            for (size_t i = 0; i < keep; ++i)
                for (int c = 0; c < channels; ++c) wav[i * channels + c] = resampled[c][drop + i];
            write_wav_f32(out, wav, out_rate, channels);
        }
        std::printf("%d buffers (%.3f s of audio) in %.3f ms on the device, %d Hz -> %s\n", n_buffers,
                    n_buffers * (double)PBSO_FRAMES_PER_BUFFER / PBSO_SAMPLE_RATE, device_ms, out_rate, out.c_str());
        return 0;
    }
    if (eq.on() && !limit) {
        // the EQ bus's output is in the WAV's scale already, and not late
        const size_t frames = sound.size() / channels;
        std::vector<float> wav(sound.size());
        for (size_t i = 0; i < frames; ++i)
            for (int c = 0; c < channels; ++c) wav[i * channels + c] = sound[(size_t)c * frames + i];
        write_wav_f32(out, wav, PBSO_SAMPLE_RATE, channels);
        std::printf("%d buffers (%.3f s of audio) in %.3f ms on the device, equalised -> %s\n", n_buffers,
                    n_buffers * (double)PBSO_FRAMES_PER_BUFFER / PBSO_SAMPLE_RATE, device_ms, out.c_str());
        return 0;
    }
    if (limit) {
        // the master bus's output is in the WAV's scale already; it is L samples late: frames L .. L + n_buffers * 513 are the file
        const size_t run = sound.size() / channels, keep = (size_t)n_buffers * PBSO_FRAMES_PER_BUFFER;
        if (pcm16) {
            write_wav_pcm16(out, std::vector<int16_t>(pcm.begin() + (size_t)lookahead * channels, pcm.begin() + ((size_t)lookahead + keep) * channels),
                            PBSO_SAMPLE_RATE, channels);
        } else {
            std::vector<float> wav(keep * channels);
            for (size_t i = 0; i < keep; ++i)
                for (int c = 0; c < channels; ++c) wav[i * channels + c] = sound[(size_t)c * run + lookahead + i];
            write_wav_f32(out, wav, PBSO_SAMPLE_RATE, channels);
        }
        std::printf("%d buffers (%.3f s of audio) in %.3f ms on the device, limited to %g -> %s\n", n_buffers,
                    n_buffers * (double)PBSO_FRAMES_PER_BUFFER / PBSO_SAMPLE_RATE, device_ms, (double)limit_T, out.c_str());
        return 0;
    }
    const size_t frames = sound.size() / channels;
    std::vector<float> frames_raw(sound.size()), wav(sound.size());
    for (size_t i = 0; i < frames; ++i)
        for (int c = 0; c < channels; ++c) frames_raw[i * channels + c] = sound[(size_t)c * frames + i];
    for (size_t i = 0; i < wav.size(); ++i) wav[i] = (float)((double)frames_raw[i] / 1E10);   // tools/...:208
    write_wav_f32(out, wav, PBSO_SAMPLE_RATE, channels);
    if (!raw.empty()) {
        FILE *f = std::fopen(raw.c_str(), "wb");
        if (!f) die("cannot write " + raw);
        std::fwrite(frames_raw.data(), 4, frames_raw.size(), f);
        std::fclose(f);
    }
    std::printf("%d buffers (%.3f s of audio) in %.3f ms on the device -> %s\n", n_buffers,
                n_buffers * (double)PBSO_FRAMES_PER_BUFFER / PBSO_SAMPLE_RATE, device_ms, out.c_str());
    return 0;
}


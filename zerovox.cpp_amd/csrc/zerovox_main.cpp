// zerovox — command-line driver, the counterpart of the reference's main() (src/zerovox.cpp:396-406):
//     ZeroVOXModel model(g_gguf_filename); model.eval(); model.write_wav_file("foo.wav");
// Run without arguments it does exactly that (model "medium-ldec.gguf", output "foo.wav", built-in utterance).
// The reference compiles its utterance in (src/zerovox.cpp:204-314: phoneme ids, punctuation ids and a style
// vector produced by a speaker encoder that is not part of the repository); here it can also be read from a text
// file so that the binary is usable with any front end:
//
//     line 1: phoneme ids            (N integers, whitespace separated)
//     line 2: punctuation ids        (N integers)
//     line 3: style embedding        (emb_dim + punct_emb_dim floats; a single 0 means the zero vector)
//
// usage: zerovox [-m model.gguf] [-u utterance.txt] [-o out.wav] [--trim] [--fit] [--info] [--plan] [prosody flags] [target flags]
//   --duration-scale S, --pitch-scale S, --pitch-shift D, --energy-scale S, --energy-shift D
//            prosody controls (include/zerovox_amd.h zv_prosody): durations * S (0 < S <= 16), pitch / energy predictions
//            p * S + D before bucketing; defaults 1, 1, 0, 1, 0 (the uncontrolled result).  A bad value is a usage error.
//   --phoneme-controls FILE
//            per-phoneme controls (include/zerovox_amd.h zv_phoneme_controls): one line per phoneme of the utterance,
//            "frames scale pitch_shift energy_shift" (frames -1 = keep the prediction, 0..32768 = exactly this many frames;
//            0 < scale <= 16; finite shifts); "-1 1 0 0" is the identity.  A wrong line count or a bad value is a usage error.
//   --alignment FILE
//            write the phoneme timings as TSV: index, phoneme_id, start_frame, frames, start_sample, samples
//   --trim   write only the frames the length regulator produced (the reference always writes max_seq_len frames,
//            src/zerovox.cpp:369)
//   --fit    fitted synthesis (include/zerovox_amd.h zv_synthesize_fitted): decode and vocode only the frames the length regulator
//            produced, and write exactly those n_frames * hop samples — the audio of the utterance at its own length, where --trim
//            cuts the file of the max_seq_len-frame run.  Works with the prosody flags, --phoneme-controls and --alignment.
//   --target-frames F, --target-seconds S
//            target durations (include/zerovox_amd.h "target durations"): the utterance's durations are fitted to sum to exactly F
//            frames, or to floor(S * sampling rate / hop size + 0.5) frames; with --fit the file holds exactly that many frames.
//            Work with --fit, the prosody flags, --phoneme-controls (forced frames stay) and --alignment.  A bad value, or a
//            target above the checkpoint's max_seq_len, is a usage error.
//   --gain-db G, --loudness-dbfs L, --peak-dbfs P
//            volume controls (include/zerovox_amd.h "volume controls"): a gain of G dB (-200 .. 60), the speech brought to an RMS
//            level of L dB re full scale (-200 .. 0), no sample above P dB re full scale (-200 .. 0); linear = 10^(dB / 20).  The
//            waveform is measured and scaled on the device; the measured rms / peak (before the gain) and the gain are printed.
//            Work with everything above.  A bad value is a usage error.
//   --phoneme-gain-db FILE, --ramp-frames R, --fade-in-ms X, --fade-out-ms X
//            amplitude envelope (include/zerovox_amd.h "amplitude envelope"): FILE holds one gain in dB per phoneme of the utterance, one
//            per line (-200 .. 24.08, linear = 10^(dB / 20) <= 16); neighbouring phonemes cross-fade over 2R + 2 frames (0 <= R <= 64);
//            the speech fades in / out over floor(X * sampling rate / 1000 + 0.5) samples (0 <= X <= 600000).  Applied on the device
//            ahead of the volume controls.  Work with everything above.  A wrong line count or a bad value is a usage error.
//   --contour FILE, --phoneme-levels FILE
//            level contour (include/zerovox_amd.h "level contour"): the level and peak of every frame of the capacity (max_seq_len rows,
//            also with --trim and --fit) / of every phoneme, metered on the device on the waveform that is written, as TSV: a header
//            line, then index<TAB>rms<TAB>peak per row, linear re full scale, printed with %.9g (the f32 bits survive).  Work with
//            everything above.  A missing file name is a usage error.
//   --pitch FILE, --phoneme-pitch FILE, --pitch-min-hz F, --pitch-max-hz F, --pitch-threshold X
//            pitch track (include/zerovox_amd.h "pitch track"): the fundamental frequency and the correlation strength of every frame of
//            the capacity / the mean F0 of the voiced frames and their share for every phoneme, metered on the device on the waveform
//            that is written, as TSV: a header line, then index<TAB>f0_hz<TAB>strength (frames) or index<TAB>f0_hz<TAB>voiced (phonemes)
//            per row, printed with %.9g.  The range in Hz becomes lags on the host, min_lag = floor(rate / max-hz) and max_lag =
//            floor(rate / min-hz) (defaults: the library's, 63 .. 441 Hz at 22 050 Hz); the threshold is the voicing threshold in
//            (0, 1], default 0.5.  A frequency that is not positive and finite, or a parameter without a file, is a usage error; the
//            library checks the lags.
//   --bands FILE, --phoneme-bands FILE, --band-edges-hz a,b,c,...
//            band levels (include/zerovox_amd.h "band levels"): the level per frequency band of every frame of the capacity / of every
//            phoneme, metered on the device on the waveform that is written, as TSV: a header line (index, then each band's range in
//            bins as lo-hi), then index<TAB>level... per row, linear re full scale, printed with %.9g.  The edges in Hz (2 .. 65
//            ascending values) become bins of the 1 024-point transform on the host, round(hz * 1024 / rate); without them the
//            library's 16 default bands.  Edges that are not ascending positive numbers, or that come without a file, are a usage
//            error; edges that fall on the same bin after rounding are refused once the checkpoint's rate is known.
//   --eq-gain-db g0,g1,..., --eq-edges-hz a,b,c,..., --eq-taps L, --filter-taps FILE
//            waveform filter (include/zerovox_amd.h "waveform filter"): a linear-phase FIR applied on the device ahead of the envelope,
//            the volume controls and every meter above.  --eq-gain-db gives a gain in dB per band (1 .. 64 finite numbers; without
//            --eq-edges-hz 16 of them, for the default bands of --bands); --eq-edges-hz the bands' edges, converted like
//            --band-edges-hz; --eq-taps the tap count (odd, 1 .. 511, default 255).  The taps come from zv_filter_design.
//            --filter-taps FILE reads the taps themselves, one per line, and excludes the other three.  A malformed value, a gain
//            count that does not match the bands, or edges / a tap count without gains are usage errors; the library checks the taps.
//   --analyze IN.wav, --mel-out FILE, --resynth OUT.wav, --mel-fmin HZ, --mel-fmax HZ, --mel-centre SAMPLE, --mel-pad reflect|zero
//            mel analysis (include/zerovox_amd.h "mel analysis") in place of synthesis: the log-mel rows (natural logarithm, Slaney
//            weights) of a mono PCM16 RIFF file at the model's rate — what zv_write_wav writes — as raw f32 [frames][mel channels], and /
//            or the vocoder's waveform of those rows.  A file at another rate or with more channels is an error by name; nothing is
//            resampled.  The mel flags without --analyze, or --analyze without an output, are usage errors.
//   --align A.f32 B.f32, --mel-width M, --align-scale S, --align-normalise, --map-out FILE
//            mel alignment (include/zerovox_amd.h "mel alignment") in place of synthesis: the dynamic-time-warping path between two
//            files of raw f32 rows [frames][M] (what --mel-out writes), printed as total, path length and distance; --map-out writes
//            the two frame maps as TSV.  --mel-width is required (1 .. 256); a file that cannot be opened, holds no whole rows or more
//            than 4 096 of them is an error by name ahead of the checkpoint.  The other four flags without --align are usage errors.
//   --loudness IN.wav, --lufs L, --true-peak-dbtp P
//            --loudness: no synthesis; the BS.1770 report (zv_loudness_wave) of a mono PCM16 RIFF file at the model's rate: integrated,
//            momentary-maximum and short-term-maximum loudness in LUFS, true peak in dBTP, sample peak, the block counts, and the gain
//            --lufs / --true-peak-dbtp would apply.  Without --loudness the two flags normalise a synthesis run: the finished waveform
//            (what -o receives) passes through the call before it is written.  --lufs in [-70, 0], --true-peak-dbtp <= 0;
//            --true-peak-dbtp alone is a ceiling without a target.  A bad value is a usage error.
//   --limit [IN.wav], --limit-dbtp P, --limit-gain-db G, --limit-attack-ms A, --limit-release-ms R
//            --limit IN.wav -o OUT.wav: no synthesis; a mono PCM16 RIFF file at the model's rate through the look-ahead peak limiter
//            (zv_limit_wave): G dB of gain (default 0) ahead of it, a ceiling of P dBTP (required, <= 0), windows of A and R ms (default
//            1.5 and 60); the report is printed and the limited waveform written.  --limit without a file, together with --lufs L
//            --true-peak-dbtp P on a synthesis run, meets the ceiling with the limiter instead of backing the gain off: the gain of the
//            target alone goes ahead of the limiter, and the loudness of what was written is printed too.  A bad value is a usage error.
//   --resample IN.wav, --rate R, --resample-zeros Z, --resample-beta B, --resample-cutoff C, --dither, --dither-seed N, --out-rate R
//            --resample IN.wav -o OUT.wav --rate R: no synthesis; a mono PCM16 RIFF file at ANY rate brought to R Hz (zv_resample_wave:
//            the design of zeros Z, beta B, cutoff C; 0 or absent: 32, 9, 0.91) and written as the device's PCM16 samples, with TPDF
//            dither under seed N where --dither is given.  This is how a recording at 44.1 or 48 kHz reaches --analyze, --loudness,
//            --limit and --time-like, which keep their refusal of another rate.  --out-rate R [--dither] on a synthesis run is the
//            last step behind --lufs / --limit: what -o would receive goes through the same call and the file is written at R Hz from
//            the device's int16 samples.  --rate without --resample, --resample without --rate, the design flags without either mode
//            and a bad value are usage errors.
//   --time-like REF.wav
//            with the synthesis flags: the utterance with the timing of the reference, a mono PCM16 RIFF file at the model's rate.
//            The utterance is synthesised (fitted), its mel rows are aligned to the reference's, the phoneme boundaries move onto the
//            reference's clock and the utterance is synthesised again with those durations; the reference's whole hops are written.
//            It excludes --align, --analyze, --phoneme-controls and the two targets.
//   --info   list the checkpoint's tensors (name, type, shape), then exit (no GPU needed)
//   --plan   print the frame count of every utterance of the -u file (which may then hold several, three lines each) without decoding
//            or vocoding, one line each: index n_phonemes n_frames seconds; the prosody flags apply to every utterance, then exit
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "zerovox.h"

static const char *k_default_model = "medium-ldec.gguf";        // reference src/zerovox.cpp:16
static const char *k_default_out = "foo.wav";                   // reference src/zerovox.cpp:403

static void usage(FILE *f)
{
    fprintf(f, "usage: zerovox [-m model.gguf] [-u utterance.txt] [-o out.wav] [--trim] [--fit] [--info] [--plan]\n"
               "               [--duration-scale S] [--pitch-scale S] [--pitch-shift D] [--energy-scale S] [--energy-shift D]\n"
               "               [--phoneme-controls FILE] [--alignment FILE] [--target-frames F | --target-seconds S]\n"
               "               [--gain-db G] [--loudness-dbfs L] [--peak-dbfs P]\n"
               "               [--phoneme-gain-db FILE] [--ramp-frames R] [--fade-in-ms X] [--fade-out-ms X]\n"
               "               [--contour FILE] [--phoneme-levels FILE]\n"
               "               [--pitch FILE] [--phoneme-pitch FILE] [--pitch-min-hz F] [--pitch-max-hz F] [--pitch-threshold X]\n"
               "               [--bands FILE] [--phoneme-bands FILE] [--band-edges-hz a,b,c,...]\n"
               "               [--eq-gain-db g0,g1,...] [--eq-edges-hz a,b,c,...] [--eq-taps L] [--filter-taps FILE]\n"
               "       zerovox -m model.gguf --analyze in.wav [--mel-out rows.f32] [--resynth out.wav]\n"
               "               [--mel-fmin HZ] [--mel-fmax HZ] [--mel-centre SAMPLE] [--mel-pad reflect|zero]\n"
               "       zerovox -m model.gguf --align a.f32 b.f32 --mel-width M [--align-scale S] [--align-normalise] [--map-out map.tsv]\n"
               "       zerovox -m model.gguf --loudness in.wav [--lufs L] [--true-peak-dbtp P]\n"
               "       zerovox -m model.gguf --limit in.wav -o out.wav --limit-dbtp P [--limit-gain-db G] [--limit-attack-ms A] [--limit-release-ms R]\n"
               "       zerovox -m model.gguf --resample in.wav -o out.wav --rate R [--resample-zeros Z] [--resample-beta B] [--resample-cutoff C]\n"
               "               [--dither] [--dither-seed N]\n"
               "       zerovox ... --lufs L [--true-peak-dbtp P]   (with the synthesis flags)\n"
               "       zerovox ... --out-rate R [--dither] [--dither-seed N]   (with the synthesis flags)\n"
               "       zerovox ... --time-like ref.wav   (with the synthesis flags)\n"
               "  defaults: -m %s -o %s, built-in utterance (like the reference's main)\n"
               "  utterance.txt: line 1 phoneme ids, line 2 punctuation ids, line 3 style floats (or a single 0)\n"
               "  --duration-scale S   every phoneme's duration times S (0 < S <= 16; 2 = twice as slow), default 1\n"
               "  --pitch-scale S      pitch prediction p -> p * S + shift before bucketing, default 1\n"
               "  --pitch-shift D      (see --pitch-scale), default 0\n"
               "  --energy-scale S     energy prediction e -> e * S + shift before bucketing, default 1\n"
               "  --energy-shift D     (see --energy-scale), default 0\n"
               "  --phoneme-controls FILE  one line per phoneme: frames scale pitch_shift energy_shift (identity: -1 1 0 0;\n"
               "                       frames -1 keeps the prediction, 0..32768 forces it; 0 < scale <= 16)\n"
               "  --alignment FILE     write the phoneme timings as TSV: index phoneme_id start_frame frames start_sample samples\n"
               "  --trim               write only the frames the length regulator produced (cut from the max_seq_len-frame run)\n"
               "  --plan               print index n_phonemes n_frames seconds per utterance of the -u file (three lines each), then exit\n"
               "  --fit                synthesize only those frames (the utterance at its own length) and write them\n"
               "  --target-frames F    fit the durations to exactly F frames (1 <= F <= the checkpoint's max_seq_len)\n"
               "  --target-seconds S   the same for floor(S * sampling rate / hop size + 0.5) frames (S > 0)\n"
               "  --gain-db G          multiply the waveform by 10^(G / 20) (-200 <= G <= 60)\n"
               "  --loudness-dbfs L    bring the speech to an RMS level of L dB re full scale (-200 <= L <= 0)\n"
               "  --peak-dbfs P        keep every sample at or under P dB re full scale (-200 <= P <= 0); prints rms / peak / gain\n"
               "  --phoneme-gain-db FILE  one gain in dB per phoneme, one per line (-200 <= dB <= 24.08: a linear gain of at most 16)\n"
               "  --ramp-frames R      cross-fade neighbouring phonemes' gains over 2R + 2 frames (0 <= R <= 64), default 0\n"
               "  --fade-in-ms X       the speech rises linearly from 0 over floor(X * sampling rate / 1000 + 0.5) samples\n"
               "  --fade-out-ms X      the speech falls linearly to 0 over as many samples; what follows it is silence\n"
               "  --contour FILE       write the level of every frame of the written waveform's capacity as TSV: index rms peak\n"
               "  --phoneme-levels FILE  write the level of every phoneme likewise\n"
               "  --pitch FILE         write the fundamental frequency of every frame of the capacity as TSV: index f0_hz strength\n"
               "  --phoneme-pitch FILE write every phoneme's mean F0 and share of voiced frames as TSV: index f0_hz voiced\n"
               "  --pitch-min-hz F, --pitch-max-hz F  the range searched (default 63 .. 441 Hz at 22 050 Hz, three octaves at most)\n"
               "  --pitch-threshold X  the correlation strength from which a frame counts as voiced, 0 < X <= 1, default 0.5\n"
               "  --bands FILE         write the level per frequency band of every frame of the capacity as TSV: index level...\n"
               "  --phoneme-bands FILE write the level per frequency band of every phoneme likewise\n"
               "  --band-edges-hz a,b,c,...  the bands' edges in Hz, 2 .. 65 ascending values (default: 16 bands, 22 Hz .. Nyquist at 22 050 Hz)\n"
               "  --eq-gain-db g0,g1,...  filter the waveform on the device: a gain in dB per band (16 for the default bands of --bands)\n"
               "  --eq-edges-hz a,b,c,...  the equaliser's band edges in Hz, converted like --band-edges-hz\n"
               "  --eq-taps L          the equaliser's tap count, odd, 1 .. 511, default 255 (a band step takes about 4096 / (L + 1) bins)\n"
               "  --filter-taps FILE   filter the waveform with the taps in FILE, one per line (an odd count of 1 .. 511), instead\n"
               "  --analyze IN.wav     no synthesis: the log-mel rows (natural logarithm) of a mono PCM16 file at the model's rate, with\n"
               "                       --mel-out FILE (raw f32 [frames][mel channels]) and / or --resynth OUT.wav (the vocoder's waveform of them);\n"
               "                       --mel-fmin HZ, --mel-fmax HZ (default 0 .. Nyquist), --mel-centre SAMPLE (0 .. hop - 1, default 0),\n"
               "                       --mel-pad reflect|zero (default reflect)\n"
               "  --align A.f32 B.f32  no synthesis: the dynamic-time-warping path between two files of raw f32 rows [frames][M] (--mel-out's\n"
               "                       format); prints total, path length and distance.  --mel-width M (1 .. 256, required), --align-scale S\n"
               "                       (steps per unit of the rows, default 64), --align-normalise (remove every channel's mean per file),\n"
               "                       --map-out FILE (TSV: side index frame, the first frame of the other file on the path)\n"
               "  --loudness IN.wav    no synthesis: the ITU-R BS.1770 report of a mono PCM16 file at the model's rate: integrated, momentary and\n"
               "                       short-term loudness (LUFS), true peak (dBTP), and the gain --lufs / --true-peak-dbtp would apply\n"
               "  --lufs L             bring the finished waveform to L LUFS integrated (-70 .. 0) before it is written\n"
               "  --true-peak-dbtp P   keep its true peak at or below P dBTP (P <= 0); with --lufs the ceiling wins\n"
               "  --resample IN.wav    no synthesis: a mono PCM16 file at any rate brought to --rate R Hz on the device and written as PCM16;\n"
               "                       --resample-zeros Z (4 .. 64, default 32), --resample-beta B ((0, 20], default 9), --resample-cutoff C\n"
               "                       ((0, 1], default 0.91), --dither (TPDF, +-1 LSB), --dither-seed N (default 0)\n"
               "  --out-rate R         write the finished waveform at R Hz, converted on the device (the last step behind --lufs / --limit)\n"
               "  --time-like REF.wav  synthesise with the timing of REF.wav (mono PCM16 at the model's rate): the phoneme boundaries of a\n"
               "                       first synthesis are moved onto the reference's clock along the alignment of the two mels\n",
            k_default_model, k_default_out);
}

template <typename T> static std::vector<T> parse_line(const std::string &line)
{
    std::vector<T> v;
    std::istringstream is(line);
    T x;
    while (is >> x) v.push_back(x);
    if (!is.eof()) throw std::runtime_error("utterance file: malformed number in '" + line.substr(0, 40) + "'");
    return v;
}

// a whole-string finite float, else a usage error (exit 2)
static float parse_flag_float(const char *flag, const std::string &v)
{
    char *end = nullptr;
    const float x = strtof(v.c_str(), &end);
    if (v.empty() || end != v.c_str() + v.size() || !std::isfinite(x))
    {
        fprintf(stderr, "zerovox: %s needs a finite number, got '%s'\n", flag, v.c_str());
        usage(stderr);
        exit(2);
    }
    return x;
}

// --phoneme-controls FILE for an utterance of n phonemes: a usage error (exit 2) on a wrong line count or a bad value
struct PhonemeControlFile
{
    std::vector<int32_t> frames;
    std::vector<float>   scale, pitch, energy;
};

static PhonemeControlFile read_phoneme_controls(const std::string &path, size_t n)
{
    auto bad = [&](const std::string &what) {
        fprintf(stderr, "zerovox: --phoneme-controls %s: %s\n", path.c_str(), what.c_str());
        usage(stderr);
        exit(2);
    };
    std::ifstream f(path);
    if (!f) bad("cannot open the file");
    PhonemeControlFile pc;
    std::string line;
    size_t lineno = 0;
    while (std::getline(f, line))
    {
        lineno++;
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;       // blank lines carry no phoneme
        std::istringstream is(line);
        std::vector<std::string> tok;
        std::string t;
        while (is >> t) tok.push_back(t);
        const std::string where = "line " + std::to_string(lineno);
        if (tok.size() != 4) bad(where + ": needs 4 values (frames scale pitch_shift energy_shift), got " + std::to_string(tok.size()));
        char *end = nullptr;
        const long fr = strtol(tok[0].c_str(), &end, 10);
        if (end != tok[0].c_str() + tok[0].size() || fr < -1 || fr > 32768) bad(where + ": frames '" + tok[0] + "' is not an integer in [-1, 32768]");
        float v[3];
        for (int k = 0; k < 3; k++)
        {
            v[k] = strtof(tok[k + 1].c_str(), &end);
            if (end != tok[k + 1].c_str() + tok[k + 1].size() || !std::isfinite(v[k])) bad(where + ": '" + tok[k + 1] + "' is not a finite number");
        }
        if (!(v[0] > 0.0f && v[0] <= 16.0f)) bad(where + ": scale " + tok[1] + " is outside (0, 16]");
        pc.frames.push_back((int32_t)fr);
        pc.scale.push_back(v[0]);
        pc.pitch.push_back(v[1]);
        pc.energy.push_back(v[2]);
    }
    if (pc.frames.size() != n)
        bad(std::to_string(pc.frames.size()) + " lines, the utterance has " + std::to_string(n) + " phonemes");
    return pc;
}

// --phoneme-gain-db FILE for an utterance of n phonemes, as linear gains: a usage error (exit 2) on a wrong line count or a bad value
static std::vector<float> read_phoneme_gains(const std::string &path, size_t n)
{
    auto bad = [&](const std::string &what) {
        fprintf(stderr, "zerovox: --phoneme-gain-db %s: %s\n", path.c_str(), what.c_str());
        usage(stderr);
        exit(2);
    };
    std::ifstream f(path);
    if (!f) bad("cannot open the file");
    std::vector<float> gains;
    std::string line;
    size_t lineno = 0;
    while (std::getline(f, line))
    {
        lineno++;
        const size_t a = line.find_first_not_of(" \t\r"), b = line.find_last_not_of(" \t\r");
        if (a == std::string::npos) continue;                                      // blank lines carry no phoneme
        const std::string tok = line.substr(a, b - a + 1), where = "line " + std::to_string(lineno);
        char *end = nullptr;
        const double db = strtod(tok.c_str(), &end);
        if (end != tok.c_str() + tok.size() || !std::isfinite(db)) bad(where + ": '" + tok + "' is not a finite number");
        const float lin = (float)pow(10.0, db / 20.0);
        if (!(db >= -200.0 && lin <= 16.0f)) bad(where + ": " + tok + " dB is outside [-200, 24.08]");
        gains.push_back(lin);
    }
    if (gains.size() != n) bad(std::to_string(gains.size()) + " lines, the utterance has " + std::to_string(n) + " phonemes");
    return gains;
}

// the utterance's phoneme ids before the model is loaded: line 1 of the utterance file, or the built-in utterance
static std::vector<int32_t> utterance_ids(const std::string &utt_path)
{
    if (utt_path.empty())
    {
        const int32_t *ids = nullptr;
        uint32_t n = 0;
        zv_demo_utterance(&ids, nullptr, nullptr, &n, nullptr);
        return std::vector<int32_t>(ids, ids + n);
    }
    std::ifstream f(utt_path);
    std::string l1;
    if (!f || !std::getline(f, l1)) throw std::runtime_error("cannot read utterance file '" + utt_path + "'");
    return parse_line<int32_t>(l1);
}

// --plan: the frame counts of the utterances in the -u file (three lines each, one utterance after the other; without -u the built-in
// one), from one zv_encode_batch call without hidden: nothing is decoded or vocoded.  One line per utterance on stdout:
// index n_phonemes n_frames seconds.  prosody: the flags' controls for every utterance, or null
static int plan(const std::string &model_path, const std::string &utt_path, const zv_prosody *prosody)
{
    zv_model *m = nullptr;
    if (zv_model_load(model_path.c_str(), 0, &m) != ZV_OK) throw std::runtime_error(zv_last_error());
    struct Free { zv_model *m; ~Free() { zv_model_free(m); } } free_model{m};
    zv_hparams hp;
    if (zv_model_get_hparams(m, &hp) != ZV_OK) throw std::runtime_error(zv_last_error());
    const size_t E = hp.emb_dim + hp.punct_emb_dim;
    std::vector<std::vector<int32_t>> ids, puncts;
    std::vector<std::vector<float>> styles;
    if (utt_path.empty())
    {
        const int32_t *i0, *p0;
        const float *s0;
        uint32_t n = 0, ns = 0;
        zv_demo_utterance(&i0, &p0, &s0, &n, &ns);
        ids.emplace_back(i0, i0 + n), puncts.emplace_back(p0, p0 + n), styles.emplace_back(s0, s0 + ns);
    }
    else
    {
        std::ifstream f(utt_path);
        if (!f) throw std::runtime_error("cannot open utterance file '" + utt_path + "'");
        std::vector<std::string> lines;
        for (std::string line; std::getline(f, line);)
            if (line.find_first_not_of(" \t\r") != std::string::npos) lines.push_back(line);
        if (lines.empty() || lines.size() % 3) throw std::runtime_error("utterance file needs three lines (ids, punctuation ids, style) per utterance");
        for (size_t k = 0; k < lines.size(); k += 3)
        {
            ids.push_back(parse_line<int32_t>(lines[k])), puncts.push_back(parse_line<int32_t>(lines[k + 1]));
            styles.push_back(parse_line<float>(lines[k + 2]));
            if (styles.back().size() == 1 && styles.back()[0] == 0.0f) styles.back().assign(E, 0.0f);
        }
    }
    const uint32_t n_utt = (uint32_t)ids.size();
    std::vector<const int32_t *> pi(n_utt), pp(n_utt);
    std::vector<const float *> ps(n_utt);
    std::vector<uint32_t> n(n_utt), T(n_utt, hp.max_seq_len), nf(n_utt, 0);
    std::vector<zv_prosody> pro(n_utt, prosody ? *prosody : zv_prosody{1.0f, 1.0f, 0.0f, 1.0f, 0.0f});
    for (uint32_t u = 0; u < n_utt; u++)
    {
        if (ids[u].empty() || ids[u].size() != puncts[u].size())
            throw std::runtime_error("utterance " + std::to_string(u) + ": need as many punctuation ids as phoneme ids (> 0)");
        if (styles[u].size() != E)
            throw std::runtime_error("utterance " + std::to_string(u) + ": style vector has " + std::to_string(styles[u].size()) + " values, model needs " + std::to_string(E));
        pi[u] = ids[u].data(), pp[u] = puncts[u].data(), ps[u] = styles[u].data(), n[u] = (uint32_t)ids[u].size();
    }
    if (zv_encode_batch(m, n_utt, pi.data(), pp.data(), ps.data(), n.data(), T.data(), nullptr, nf.data(), prosody ? pro.data() : nullptr, nullptr,
                        nullptr, nullptr) != ZV_OK)
        throw std::runtime_error(zv_last_error());
    for (uint32_t u = 0; u < n_utt; u++)
        printf("%u %u %u %.3f\n", u, n[u], nf[u], (double)nf[u] * hp.audio_hop_size / hp.audio_sampling_rate);
    return 0;
}

// --analyze IN.wav: the file's log-mel rows (zv_mel_wave: natural logarithm, Slaney weights fmin .. fmax, the model's hop and channel
// count) as raw little-endian f32 [T][num_mels] in --mel-out, and with --resynth OUT.wav the vocoder's waveform of those rows.  The
// file must be what zv_write_wav writes: mono PCM16 RIFF at the model's rate; anything else is an error by name, nothing is resampled.
// Samples behind the last whole hop are dropped.
// a mono PCM16 RIFF file's samples as floats (what zv_write_wav writes), refused by the flag's name otherwise
static std::vector<float> read_pcm16(const std::string &flag, const std::string &in_path, uint32_t &rate)
{
    std::ifstream f(in_path, std::ios::binary);
    if (!f) throw std::runtime_error(flag + ": cannot open '" + in_path + "'");
    const std::vector<unsigned char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    auto u16 = [&](size_t o) { return (uint32_t)b[o] | (uint32_t)b[o + 1] << 8; };
    auto u32 = [&](size_t o) { return u16(o) | u16(o + 2) << 16; };
    if (b.size() < 12 || memcmp(b.data(), "RIFF", 4) != 0 || memcmp(b.data() + 8, "WAVE", 4) != 0)
        throw std::runtime_error(flag + ": '" + in_path + "' is not a RIFF/WAVE file");
    uint32_t format = 0, channels = 0, bits = 0;
    size_t data = 0, data_bytes = 0;
    rate = 0;
    for (size_t o = 12; o + 8 <= b.size();)
    {
        const size_t n = u32(o + 4), body = o + 8;
        if (!memcmp(b.data() + o, "fmt ", 4) && n >= 16 && body + 16 <= b.size())
            format = u16(body), channels = u16(body + 2), rate = u32(body + 4), bits = u16(body + 14);
        if (!memcmp(b.data() + o, "data", 4))
        {
            data = body, data_bytes = std::min(n, b.size() - body);
            break;
        }
        o = body + n + (n & 1);
    }
    if (!rate || !data) throw std::runtime_error(flag + ": '" + in_path + "' has no fmt or no data chunk");
    if (format != 1 || bits != 16) throw std::runtime_error(flag + ": '" + in_path + "' is not 16-bit PCM (format " + std::to_string(format) + ", " + std::to_string(bits) + " bits)");
    if (channels != 1) throw std::runtime_error(flag + ": '" + in_path + "' has " + std::to_string(channels) + " channels, mono is needed");
    std::vector<float> x(data_bytes / 2);
    for (size_t i = 0; i < x.size(); i++) x[i] = (float)(int16_t)u16(data + 2 * i) / 32768.0f;
    return x;
}

static int analyze(const std::string &model_path, const std::string &in_path, const std::string &mel_path, const std::string &resynth_path,
                   const zv_mel &q)
{
    uint32_t rate = 0;
    const std::vector<float> pcm = read_pcm16("--analyze", in_path, rate);
    zv_model *m = nullptr;
    if (zv_model_load(model_path.c_str(), 0, &m) != ZV_OK) throw std::runtime_error(zv_last_error());
    struct Free { zv_model *m; ~Free() { zv_model_free(m); } } free_model{m};
    zv_hparams hp;
    if (zv_model_get_hparams(m, &hp) != ZV_OK) throw std::runtime_error(zv_last_error());
    if (rate != hp.audio_sampling_rate)
        throw std::runtime_error("--analyze: '" + in_path + "' is at " + std::to_string(rate) + " Hz, the model at " + std::to_string(hp.audio_sampling_rate) + " Hz (nothing is resampled)");
    const size_t T = pcm.size() / hp.audio_hop_size;
    if (T == 0 || T > zv_max_frames(m))
        throw std::runtime_error("--analyze: '" + in_path + "' holds " + std::to_string(T) + " frames of " + std::to_string(hp.audio_hop_size) + " samples, 1 .. " + std::to_string(zv_max_frames(m)) + " are needed");
    std::vector<float> wav(pcm.begin(), pcm.begin() + T * hp.audio_hop_size), mel(T * hp.audio_num_mels);
    if (zv_mel_wave(m, wav.data(), (uint32_t)T, &q, mel.data()) != ZV_OK) throw std::runtime_error(zv_last_error());
    if (!mel_path.empty())
    {
        std::ofstream o(mel_path, std::ios::binary);
        o.write((const char *)mel.data(), (std::streamsize)(mel.size() * 4));
        if (!o) throw std::runtime_error("--mel-out: cannot write '" + mel_path + "'");
    }
    printf("%s: %zu frames x %u mel channels\n", in_path.c_str(), T, hp.audio_num_mels);
    if (!resynth_path.empty())
    {
        if (zv_vocode(m, mel.data(), (uint32_t)T, wav.data()) != ZV_OK) throw std::runtime_error(zv_last_error());
        if (zv_write_wav(resynth_path.c_str(), wav.data(), wav.size(), hp.audio_sampling_rate) != ZV_OK) throw std::runtime_error(zv_last_error());
    }
    return 0;
}

static void print_loudness(const char *what, const zv_loudness_result &r)
{
    printf("%s: integrated %.2f LUFS, momentary max %.2f LUFS, short-term max %.2f LUFS, true peak %.2f dBTP (sample peak %.6f), "
           "blocks %u / %u / %u, gain %.6f\n",
           what, (double)r.integrated_lufs, (double)r.momentary_max_lufs, (double)r.short_term_max_lufs, (double)r.true_peak_dbtp,
           (double)r.sample_peak, r.blocks, r.blocks_absolute, r.blocks_gated, (double)r.gain);
}

// --loudness IN.wav: the file's BS.1770 report (zv_loudness_wave, a meter: nothing is written); the file as for --analyze
static void print_limit(const char *what, const zv_limit_result &r)
{
    printf("%s: true peak %.2f dBTP before, %.2f dBTP after (sample peak %.6f before, %.6f after), least gain %.6f (%.2f dB), "
           "limited samples %llu\n",
           what, (double)r.true_peak_before_dbtp, (double)r.true_peak_after_dbtp, (double)r.sample_peak_before, (double)r.sample_peak_after,
           (double)r.min_gain, (double)r.reduction_db, (unsigned long long)r.limited_samples);
}

// what --limit-dbtp, --limit-gain-db and the two windows ask for at a rate
struct LimitFlags { float dbtp = 0.0f, gain_db = 0.0f, attack_ms = 0.0f, release_ms = 0.0f; bool have_dbtp = false; };
static zv_limiter limit_ask(const LimitFlags &f, uint32_t rate, float gain, float ceiling)
{
    zv_limiter q = {gain, ceiling, 0u, 0u, 0u};
    if (zv_limit_design(rate, f.attack_ms, f.release_ms, &q.attack, &q.release) != ZV_OK) throw std::runtime_error(zv_last_error());
    return q;
}

// --limit IN.wav -o OUT.wav: the file through zv_limit_wave; the file as for --analyze
static int limit_file(const std::string &model_path, const std::string &in_path, const std::string &out_path, const LimitFlags &f)
{
    uint32_t rate = 0;
    const std::vector<float> pcm = read_pcm16("--limit", in_path, rate);
    zv_model *m = nullptr;
    if (zv_model_load(model_path.c_str(), 0, &m) != ZV_OK) throw std::runtime_error(zv_last_error());
    struct Free { zv_model *m; ~Free() { zv_model_free(m); } } free_model{m};
    zv_hparams hp;
    if (zv_model_get_hparams(m, &hp) != ZV_OK) throw std::runtime_error(zv_last_error());
    if (rate != hp.audio_sampling_rate)
        throw std::runtime_error("--limit: '" + in_path + "' is at " + std::to_string(rate) + " Hz, the model at " + std::to_string(hp.audio_sampling_rate) + " Hz (nothing is resampled)");
    const size_t T = pcm.size() / hp.audio_hop_size;
    if (T == 0 || T > zv_max_frames(m))
        throw std::runtime_error("--limit: '" + in_path + "' holds " + std::to_string(T) + " frames of " + std::to_string(hp.audio_hop_size) + " samples, 1 .. " + std::to_string(zv_max_frames(m)) + " are needed");
    const zv_limiter q = limit_ask(f, rate, (float)pow(10.0, (double)f.gain_db / 20.0), (float)pow(10.0, (double)f.dbtp / 20.0));
    std::vector<float> out(T * hp.audio_hop_size);
    zv_limit_result r;
    if (zv_limit_wave(m, pcm.data(), (uint32_t)T, (uint32_t)T, &q, &r, out.data()) != ZV_OK) throw std::runtime_error(zv_last_error());
    print_limit(in_path.c_str(), r);
    if (zv_write_wav(out_path.c_str(), out.data(), out.size(), hp.audio_sampling_rate) != ZV_OK) throw std::runtime_error(zv_last_error());
    printf("Successfully created %s with %zu samples (%zu frames).\n", out_path.c_str(), out.size(), T);
    return 0;
}

// what --rate / --out-rate, the design flags and the dither flags ask for
struct ResampleFlags { uint32_t rate = 0, zeros = 0, seed = 0; float beta = 0.0f, cutoff = 0.0f; bool dither = false, design = false, seeded = false; };
static zv_resample resample_ask(const ResampleFlags &f, uint32_t rate_in)
{
    zv_resample q{};
    q.rate_in = rate_in, q.rate_out = f.rate, q.zeros = f.zeros, q.beta = f.beta, q.cutoff = f.cutoff;
    q.flags = f.dither ? 1u : 0u, q.seed = f.seed;
    return q;
}
static void print_resample(const char *what, const zv_resample &q, uint64_t S_in, const zv_resample_result &r)
{
    uint32_t L = 0, M = 0, P = 0;
    if (zv_resample_design(q.rate_in, q.rate_out, q.zeros, q.beta, q.cutoff, &L, &M, &P, nullptr) != ZV_OK) throw std::runtime_error(zv_last_error());
    printf("%s: %u -> %u Hz (L %u, M %u, %u taps per phase), %llu -> %llu samples, sample peak %.6f, clipped %llu%s\n", what, q.rate_in, q.rate_out, L, M, P,
           (unsigned long long)S_in, (unsigned long long)r.n_out, (double)r.sample_peak, (unsigned long long)r.clipped, q.flags ? ", dithered" : "");
}
// S_in samples as PCM16 at the ask's rate, written to out_path: `call(ask, pcm)` is the resampling call (the C-ABI's or the facade's)
// over those samples; no samples give an empty file
template <typename Call> static zv_resample_result resample_to_file(const char *what, uint64_t S_in, const zv_resample &q, const std::string &out_path, Call call)
{
    uint32_t L = 0, M = 0, P = 0;
    if (zv_resample_design(q.rate_in, q.rate_out, q.zeros, q.beta, q.cutoff, &L, &M, &P, nullptr) != ZV_OK) throw std::runtime_error(zv_last_error());
    std::vector<int16_t> pcm((size_t)zv_resample_count(S_in, L, M));
    zv_resample_result r{};
    if (S_in) r = call(q, pcm.data());
    print_resample(what, q, S_in, r);
    if (zv_write_wav_pcm16(out_path.c_str(), pcm.data(), pcm.size(), q.rate_out) != ZV_OK) throw std::runtime_error(zv_last_error());
    printf("Successfully created %s with %zu samples at %u Hz.\n", out_path.c_str(), pcm.size(), q.rate_out);
    return r;
}

// --resample IN.wav -o OUT.wav --rate R: a mono PCM16 RIFF file at any rate through zv_resample_wave
static int resample_file(const std::string &model_path, const std::string &in_path, const std::string &out_path, const ResampleFlags &f)
{
    uint32_t rate = 0;
    const std::vector<float> pcm = read_pcm16("--resample", in_path, rate);
    zv_model *m = nullptr;
    if (zv_model_load(model_path.c_str(), 0, &m) != ZV_OK) throw std::runtime_error(zv_last_error());
    struct Free { zv_model *m; ~Free() { zv_model_free(m); } } free_model{m};
    zv_hparams hp;
    if (zv_model_get_hparams(m, &hp) != ZV_OK) throw std::runtime_error(zv_last_error());
    const uint64_t most = (uint64_t)zv_max_frames(m) * hp.audio_hop_size;
    if (pcm.empty() || pcm.size() > most)
        throw std::runtime_error("--resample: '" + in_path + "' holds " + std::to_string(pcm.size()) + " samples, 1 .. " + std::to_string(most) + " are needed");
    resample_to_file(in_path.c_str(), pcm.size(), resample_ask(f, rate), out_path, [&](const zv_resample &q, int16_t *out) {
        zv_resample_result r{};
        if (zv_resample_wave(m, pcm.data(), pcm.size(), &q, &r, nullptr, out) != ZV_OK) throw std::runtime_error(zv_last_error());
        return r;
    });
    return 0;
}

static int loudness_file(const std::string &model_path, const std::string &in_path, const zv_loudness &q)
{
    uint32_t rate = 0;
    const std::vector<float> pcm = read_pcm16("--loudness", in_path, rate);
    zv_model *m = nullptr;
    if (zv_model_load(model_path.c_str(), 0, &m) != ZV_OK) throw std::runtime_error(zv_last_error());
    struct Free { zv_model *m; ~Free() { zv_model_free(m); } } free_model{m};
    zv_hparams hp;
    if (zv_model_get_hparams(m, &hp) != ZV_OK) throw std::runtime_error(zv_last_error());
    if (rate != hp.audio_sampling_rate)
        throw std::runtime_error("--loudness: '" + in_path + "' is at " + std::to_string(rate) + " Hz, the model at " + std::to_string(hp.audio_sampling_rate) + " Hz (nothing is resampled)");
    const size_t T = pcm.size() / hp.audio_hop_size;
    if (T == 0 || T > zv_max_frames(m))
        throw std::runtime_error("--loudness: '" + in_path + "' holds " + std::to_string(T) + " frames of " + std::to_string(hp.audio_hop_size) + " samples, 1 .. " + std::to_string(zv_max_frames(m)) + " are needed");
    zv_loudness_result r;
    if (zv_loudness_wave(m, pcm.data(), (uint32_t)T, (uint32_t)T, &q, &r, nullptr) != ZV_OK) throw std::runtime_error(zv_last_error());
    print_loudness(in_path.c_str(), r);
    return 0;
}

// --align A.f32 B.f32: the files' rows, checked ahead of the checkpoint; then zv_mel_align and the printout
static std::vector<float> read_rows(const std::string &path, uint32_t width)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("--align: cannot open '" + path + "'");
    const std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const size_t row = (size_t)width * 4;
    if (b.empty() || b.size() % row)
        throw std::runtime_error("--align: '" + path + "' holds " + std::to_string(b.size()) + " bytes, not whole rows of " + std::to_string(width) + " f32 values");
    if (b.size() / row > ZV_ALIGN_MAX_FRAMES)
        throw std::runtime_error("--align: '" + path + "' holds " + std::to_string(b.size() / row) + " rows, 1 .. " + std::to_string(ZV_ALIGN_MAX_FRAMES) + " are needed");
    std::vector<float> x(b.size() / 4);
    memcpy(x.data(), b.data(), b.size());
    return x;
}

static int align_files(const std::string &model_path, const std::string &a_path, const std::string &b_path, uint32_t width, const zv_align &q,
                       const std::string &map_path)
{
    const std::vector<float> a = read_rows(a_path, width), b = read_rows(b_path, width);
    const uint32_t Ta = (uint32_t)(a.size() / width), Tb = (uint32_t)(b.size() / width);
    ZeroVOX::ZeroVOXModel model(model_path);
    std::vector<int32_t> map_a(Ta), map_b(Tb);
    const zv_alignment r = model.align(a.data(), Ta, b.data(), Tb, width, &q, map_a.data(), map_b.data());
    printf("%s (%u rows) against %s (%u rows), %u channels: total %llu path_len %u distance %.17g\n", a_path.c_str(), Ta, b_path.c_str(), Tb, width,
           (unsigned long long)r.total, r.path_len, r.distance);
    if (!map_path.empty())
    {
        FILE *mf = fopen(map_path.c_str(), "w");
        if (!mf) throw std::runtime_error("--map-out: cannot open '" + map_path + "' for writing");
        fprintf(mf, "side\tindex\tframe\n");
        for (uint32_t i = 0; i < Ta; i++) fprintf(mf, "a\t%u\t%d\n", i, map_a[i]);
        for (uint32_t j = 0; j < Tb; j++) fprintf(mf, "b\t%u\t%d\n", j, map_b[j]);
        if (fclose(mf) != 0) throw std::runtime_error("short write to '" + map_path + "'");
    }
    return 0;
}

int main(int argc, char **argv)
{
    std::string align_a, align_b, map_path, like_path;         // --align, --map-out, --time-like
    zv_align align_q{};                                        // --align-scale, --align-normalise
    long mel_width = 0;                                        // --mel-width
    bool align_flag = false;
    std::string analyze_path, melout_path, resynth_path;      // --analyze, --mel-out, --resynth
    std::string loudness_path;                                 // --loudness
    zv_loudness loud_q = {1.0f, 0.0f, 0.0f, 0u};               // --lufs, --true-peak-dbtp
    bool limit = false;                                        // --limit
    std::string limit_path;                                    // --limit IN.wav
    LimitFlags limit_f;                                        // --limit-dbtp, --limit-gain-db, --limit-attack-ms, --limit-release-ms
    std::string resample_path;                                 // --resample IN.wav
    ResampleFlags resample_f;                                  // --rate / --out-rate, --resample-zeros, --resample-beta, --resample-cutoff, --dither, --dither-seed
    bool rate_flag = false, out_rate_flag = false;
    zv_mel mel_q{};                                            // --mel-fmin, --mel-fmax, --mel-centre, --mel-pad
    mel_q.log = 1;
    mel_q.pad = 1;
    bool mel_flag = false;
    std::string model_path = k_default_model, out_path = k_default_out, utt_path, pc_path, align_path, gain_path, contour_path, plevel_path, pitch_path, ppitch_path;
    std::string bands_path, pbands_path;
    std::vector<double> band_hz;       // --band-edges-hz
    std::vector<double> eq_hz, eq_db;  // --eq-edges-hz, --eq-gain-db
    long eq_taps = 255;                // --eq-taps
    bool eq_taps_given = false;
    std::string taps_path;             // --filter-taps
    double pitch_hz[2] = {0.0, 0.0}, pitch_thr = 0.0;      // --pitch-min-hz, --pitch-max-hz, --pitch-threshold (0: the default)
    bool pitch_param = false;
    bool trim = false, fit = false, info = false, planning = false, controlled = false, leveled = false, enveloped = false;
    long ramp_frames = 0;              // --ramp-frames
    double fade_ms[2] = {0.0, 0.0};    // --fade-in-ms, --fade-out-ms
    zv_volume volume = {1.0f, 0.0f, 0.0f};
    long target_frames = 0;            // --target-frames
    double target_seconds = 0.0;       // --target-seconds
    zv_prosody prosody = {1.0f, 1.0f, 0.0f, 1.0f, 0.0f};
    for (int i = 1; i < argc; i++)
    {
        const std::string a = argv[i];
        auto need = [&](const char *flag) -> std::string {
            if (i + 1 >= argc) { fprintf(stderr, "zerovox: %s needs a value\n", flag); usage(stderr); exit(2); }
            return argv[++i];
        };
        if (a == "-m") model_path = need("-m");
        else if (a == "-u") utt_path = need("-u");
        else if (a == "-o") out_path = need("-o");
        else if (a == "--phoneme-controls") pc_path = need("--phoneme-controls");
        else if (a == "--alignment") align_path = need("--alignment");
        else if (a == "--contour") contour_path = need("--contour");
        else if (a == "--phoneme-levels") plevel_path = need("--phoneme-levels");
        else if (a == "--pitch") pitch_path = need("--pitch");
        else if (a == "--phoneme-pitch") ppitch_path = need("--phoneme-pitch");
        else if (a == "--bands") bands_path = need("--bands");
        else if (a == "--phoneme-bands") pbands_path = need("--phoneme-bands");
        else if (a == "--band-edges-hz" || a == "--eq-edges-hz")
        {
            const std::string v = need(a.c_str());
            std::vector<double> &hz = a == "--eq-edges-hz" ? eq_hz : band_hz;
            bool ok = !v.empty();
            hz.clear();
            for (size_t at = 0; ok && at <= v.size();)
            {
                const size_t comma = std::min(v.find(',', at), v.size());
                const std::string item = v.substr(at, comma - at);
                char *end = nullptr;
                const double x = strtod(item.c_str(), &end);
                ok = !item.empty() && end == item.c_str() + item.size() && x > 0.0 && x <= 1e6 && (hz.empty() || x > hz.back());
                hz.push_back(x);
                at = comma + 1;
            }
            if (!ok || hz.size() < 2 || hz.size() > 65)
            {
                fprintf(stderr, "zerovox: %s needs 2 to 65 ascending numbers in (0, 1000000], separated by commas, got '%s'\n", a.c_str(), v.c_str());
                usage(stderr);
                return 2;
            }
        }
        else if (a == "--eq-gain-db")
        {
            const std::string v = need("--eq-gain-db");
            bool ok = !v.empty();
            eq_db.clear();
            for (size_t at = 0; ok && at <= v.size();)
            {
                const size_t comma = std::min(v.find(',', at), v.size());
                const std::string item = v.substr(at, comma - at);
                char *end = nullptr;
                const double x = strtod(item.c_str(), &end);
                ok = !item.empty() && end == item.c_str() + item.size() && std::isfinite(x);
                eq_db.push_back(x);
                at = comma + 1;
            }
            if (!ok || eq_db.size() > 64)
            {
                fprintf(stderr, "zerovox: --eq-gain-db needs 1 to 64 finite numbers separated by commas, got '%s'\n", v.c_str());
                usage(stderr);
                return 2;
            }
        }
        else if (a == "--eq-taps")
        {
            const std::string v = need("--eq-taps");
            char *end = nullptr;
            eq_taps = strtol(v.c_str(), &end, 10);
            if (v.empty() || end != v.c_str() + v.size() || eq_taps < 1 || eq_taps > 511 || eq_taps % 2 == 0)
            {
                fprintf(stderr, "zerovox: --eq-taps needs an odd number in 1 .. 511, got '%s'\n", v.c_str());
                usage(stderr);
                return 2;
            }
            eq_taps_given = true;
        }
        else if (a == "--filter-taps") taps_path = need("--filter-taps");
        else if (a == "--analyze") analyze_path = need("--analyze");
        else if (a == "--align")
        {
            if (i + 2 >= argc) { fprintf(stderr, "zerovox: --align needs two files\n"); usage(stderr); return 2; }
            align_a = argv[++i];
            align_b = argv[++i];
        }
        else if (a == "--mel-width")
        {
            const std::string v = need("--mel-width");
            char *end = nullptr;
            mel_width = strtol(v.c_str(), &end, 10);
            if (v.empty() || end != v.c_str() + v.size() || mel_width < 1 || mel_width > 256)
            {
                fprintf(stderr, "zerovox: --mel-width: '%s' is not a channel count of 1 .. 256\n", v.c_str());
                usage(stderr);
                return 2;
            }
            align_flag = true;
        }
        else if (a == "--align-scale")
        {
            align_q.scale = parse_flag_float("--align-scale", need("--align-scale"));
            if (!(align_q.scale > 0.0f))
            {
                fprintf(stderr, "zerovox: --align-scale must be positive\n");
                usage(stderr);
                return 2;
            }
            align_flag = true;
        }
        else if (a == "--align-normalise") align_q.normalise = 1, align_flag = true;
        else if (a == "--map-out") map_path = need("--map-out"), align_flag = true;
        else if (a == "--time-like") like_path = need("--time-like");
        else if (a == "--loudness") loudness_path = need("--loudness");
        else if (a == "--limit")
        {
            limit = true;
            if (i + 1 < argc && argv[i + 1][0] != '-') limit_path = argv[++i];      // (a file; without one the flag joins --lufs / --true-peak-dbtp)
        }
        else if (a == "--limit-dbtp" || a == "--limit-gain-db" || a == "--limit-attack-ms" || a == "--limit-release-ms")
        {
            const float v = parse_flag_float(a.c_str(), need(a.c_str()));
            const bool ms = a == "--limit-attack-ms" || a == "--limit-release-ms";
            if (a == "--limit-dbtp" ? !(v <= 0.0f && v >= -200.0f) : ms ? !(v > 0.0f && v <= 10000.0f) : !(v >= -200.0f && v <= 60.0f))
            {
                fprintf(stderr, "zerovox: %s %g is outside %s\n", a.c_str(), (double)v, a == "--limit-dbtp" ? "[-200, 0]" : ms ? "(0, 10000]" : "[-200, 60]");
                usage(stderr);
                return 2;
            }
            if (a == "--limit-dbtp") limit_f.dbtp = v, limit_f.have_dbtp = true;
            else if (a == "--limit-gain-db") limit_f.gain_db = v;
            else if (a == "--limit-attack-ms") limit_f.attack_ms = v;
            else limit_f.release_ms = v;
        }
        else if (a == "--resample") resample_path = need("--resample");
        else if (a == "--dither") resample_f.dither = true;
        else if (a == "--rate" || a == "--out-rate" || a == "--resample-zeros" || a == "--dither-seed")
        {
            const std::string v = need(a.c_str());
            char *end = nullptr;
            const unsigned long long n = strtoull(v.c_str(), &end, 10);
            const bool rate = a == "--rate" || a == "--out-rate";
            if (v.empty() || v[0] == '-' || end != v.c_str() + v.size() || n > 0xffffffffull || (rate && !(n >= 4000 && n <= 768000)) ||
                (a == "--resample-zeros" && !(n >= 4 && n <= 64)))
            {
                fprintf(stderr, "zerovox: %s %s is not a whole number in %s\n", a.c_str(), v.c_str(), rate ? "[4000, 768000]" : a == "--resample-zeros" ? "[4, 64]" : "[0, 4294967295]");
                usage(stderr);
                return 2;
            }
            if (rate) resample_f.rate = (uint32_t)n, (a == "--rate" ? rate_flag : out_rate_flag) = true;
            else if (a == "--resample-zeros") resample_f.zeros = (uint32_t)n, resample_f.design = true;
            else resample_f.seed = (uint32_t)n, resample_f.seeded = true;
        }
        else if (a == "--resample-beta" || a == "--resample-cutoff")
        {
            const float v = parse_flag_float(a.c_str(), need(a.c_str()));
            if (!(v > 0.0f && v <= (a == "--resample-beta" ? 20.0f : 1.0f)))
            {
                fprintf(stderr, "zerovox: %s %g is outside %s\n", a.c_str(), (double)v, a == "--resample-beta" ? "(0, 20]" : "(0, 1]");
                usage(stderr);
                return 2;
            }
            (a == "--resample-beta" ? resample_f.beta : resample_f.cutoff) = v;
            resample_f.design = true;
        }
        else if (a == "--lufs" || a == "--true-peak-dbtp")
        {
            const float v = parse_flag_float(a.c_str(), need(a.c_str()));
            if (a == "--lufs" ? !(v >= -70.0f && v <= 0.0f) : !(v <= 0.0f && v >= -200.0f))
            {
                fprintf(stderr, "zerovox: %s %g is outside %s\n", a.c_str(), (double)v, a == "--lufs" ? "[-70, 0]" : "[-200, 0]");
                usage(stderr);
                return 2;
            }
            if (a == "--lufs") loud_q.target_lufs = v, loud_q.flags |= ZV_LOUDNESS_TARGET;
            else loud_q.true_peak_ceiling = (float)pow(10.0, (double)v / 20.0), loud_q.flags |= ZV_LOUDNESS_CEILING;
        }
        else if (a == "--mel-out") melout_path = need("--mel-out"), mel_flag = true;
        else if (a == "--resynth") resynth_path = need("--resynth"), mel_flag = true;
        else if (a == "--mel-fmin") mel_q.fmin_hz = parse_flag_float("--mel-fmin", need("--mel-fmin")), mel_flag = true;
        else if (a == "--mel-fmax") mel_q.fmax_hz = parse_flag_float("--mel-fmax", need("--mel-fmax")), mel_flag = true;
        else if (a == "--mel-centre")
        {
            const std::string v = need("--mel-centre");
            char *end = nullptr;
            const long c = strtol(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || c < 0 || c > 0x7fffffffL)
            {
                fprintf(stderr, "zerovox: --mel-centre: '%s' is not a sample of a hop\n", v.c_str());
                usage(stderr);
                return 2;
            }
            mel_q.centre = (uint32_t)c, mel_flag = true;
        }
        else if (a == "--mel-pad")
        {
            const std::string v = need("--mel-pad");
            if (v != "reflect" && v != "zero")
            {
                fprintf(stderr, "zerovox: --mel-pad: '%s' is neither reflect nor zero\n", v.c_str());
                usage(stderr);
                return 2;
            }
            mel_q.pad = v == "reflect", mel_flag = true;
        }
        else if (a == "--pitch-min-hz" || a == "--pitch-max-hz" || a == "--pitch-threshold")
        {
            const std::string v = need(a.c_str());
            char *end = nullptr;
            const double x = strtod(v.c_str(), &end);
            const bool thr = a == "--pitch-threshold";
            if (v.empty() || end != v.c_str() + v.size() || !(x > 0.0 && x <= (thr ? 1.0 : 1e6)))
            {
                fprintf(stderr, "zerovox: %s needs a number in (0, %s], got '%s'\n", a.c_str(), thr ? "1" : "1000000", v.c_str());
                usage(stderr);
                return 2;
            }
            if (thr) pitch_thr = x;
            else pitch_hz[a == "--pitch-max-hz"] = x;
            pitch_param = true;
        }
        else if (a == "--target-frames")
        {
            const std::string v = need("--target-frames");
            char *end = nullptr;
            target_frames = strtol(v.c_str(), &end, 10);
            if (v.empty() || end != v.c_str() + v.size() || target_frames < 1 || target_frames > 32768)
            {
                fprintf(stderr, "zerovox: --target-frames needs an integer in [1, 32768], got '%s'\n", v.c_str());
                usage(stderr);
                return 2;
            }
            target_seconds = 0.0;
        }
        else if (a == "--target-seconds")
        {
            const std::string v = need("--target-seconds");
            char *end = nullptr;
            target_seconds = strtod(v.c_str(), &end);
            if (v.empty() || end != v.c_str() + v.size() || !std::isfinite(target_seconds) || !(target_seconds > 0.0))
            {
                fprintf(stderr, "zerovox: --target-seconds needs a finite number > 0, got '%s'\n", v.c_str());
                usage(stderr);
                return 2;
            }
            target_frames = 0;
        }
        else if (a == "--gain-db" || a == "--loudness-dbfs" || a == "--peak-dbfs")
        {
            const float db = parse_flag_float(a.c_str(), need(a.c_str()));
            const float hi = a == "--gain-db" ? 60.0f : 0.0f;
            if (!(db >= -200.0f && db <= hi))
            {
                fprintf(stderr, "zerovox: %s must be in [-200, %g] dB, got %g\n", a.c_str(), (double)hi, (double)db);
                usage(stderr);
                return 2;
            }
            const float lin = (float)pow(10.0, (double)db / 20.0);
            if (a == "--gain-db") volume.gain = lin;
            else if (a == "--loudness-dbfs") volume.target_rms = lin;
            else volume.peak_ceiling = lin;
            leveled = true;
        }
        else if (a == "--phoneme-gain-db")
        {
            gain_path = need("--phoneme-gain-db");
            enveloped = true;
        }
        else if (a == "--ramp-frames")
        {
            const std::string v = need("--ramp-frames");
            char *end = nullptr;
            ramp_frames = strtol(v.c_str(), &end, 10);
            if (v.empty() || end != v.c_str() + v.size() || ramp_frames < 0 || ramp_frames > 64)
            {
                fprintf(stderr, "zerovox: --ramp-frames needs an integer in [0, 64], got '%s'\n", v.c_str());
                usage(stderr);
                return 2;
            }
            enveloped = true;
        }
        else if (a == "--fade-in-ms" || a == "--fade-out-ms")
        {
            // a double, as written: the sample count is floor(ms * rate / 1000 + 0.5) of that double (capi.Envelope.from_db's)
            const std::string v = need(a.c_str());
            char *end = nullptr;
            const double ms = strtod(v.c_str(), &end);
            if (v.empty() || end != v.c_str() + v.size() || !(ms >= 0.0 && ms <= 600000.0))
            {
                fprintf(stderr, "zerovox: %s needs a number in [0, 600000] ms, got '%s'\n", a.c_str(), v.c_str());
                usage(stderr);
                return 2;
            }
            fade_ms[a == "--fade-out-ms"] = ms;
            enveloped = true;
        }
        else if (a == "--trim") trim = true;
        else if (a == "--fit") fit = true;
        else if (a == "--info") info = true;
        else if (a == "--plan") planning = true;
        else if (a == "--duration-scale" || a == "--pitch-scale" || a == "--pitch-shift" || a == "--energy-scale" || a == "--energy-shift")
        {
            const float x = parse_flag_float(a.c_str(), need(a.c_str()));
            if (a == "--duration-scale")
            {
                if (!(x > 0.0f && x <= 16.0f))
                {
                    fprintf(stderr, "zerovox: --duration-scale must be in (0, 16], got %g\n", (double)x);
                    usage(stderr);
                    return 2;
                }
                prosody.duration_scale = x;
            }
            else if (a == "--pitch-scale") prosody.pitch_scale = x;
            else if (a == "--pitch-shift") prosody.pitch_shift = x;
            else if (a == "--energy-scale") prosody.energy_scale = x;
            else prosody.energy_shift = x;
            controlled = true;
        }
        else if (a == "-h" || a == "--help") { usage(stdout); return 0; }
        else { fprintf(stderr, "zerovox: unknown argument '%s'\n", a.c_str()); usage(stderr); return 2; }
    }
    if (mel_flag && analyze_path.empty())
    {
        fprintf(stderr, "zerovox: --mel-out, --resynth, --mel-fmin, --mel-fmax, --mel-centre and --mel-pad need --analyze IN.wav\n");
        usage(stderr);
        return 2;
    }
    if (!analyze_path.empty() && melout_path.empty() && resynth_path.empty())
    {
        fprintf(stderr, "zerovox: --analyze needs --mel-out FILE or --resynth FILE\n");
        usage(stderr);
        return 2;
    }
    if (!loudness_path.empty() && (!analyze_path.empty() || !align_a.empty() || !like_path.empty() || planning))
    {
        fprintf(stderr, "zerovox: --loudness and --analyze, --align, --time-like, --plan exclude each other\n");
        usage(stderr);
        return 2;
    }
    if (!limit_path.empty() && (!loudness_path.empty() || !analyze_path.empty() || !align_a.empty() || !like_path.empty() || planning))
    {
        fprintf(stderr, "zerovox: --limit IN.wav and --loudness, --analyze, --align, --time-like, --plan exclude each other\n");
        usage(stderr);
        return 2;
    }
    if (!limit_path.empty() && !limit_f.have_dbtp)
    {
        fprintf(stderr, "zerovox: --limit IN.wav needs --limit-dbtp P\n");
        usage(stderr);
        return 2;
    }
    if (limit && limit_path.empty() && loud_q.flags != (ZV_LOUDNESS_TARGET | ZV_LOUDNESS_CEILING))
    {
        fprintf(stderr, "zerovox: --limit needs a file (--limit IN.wav) or, on a synthesis run, both --lufs L and --true-peak-dbtp P\n");
        usage(stderr);
        return 2;
    }
    if (!limit && (limit_f.have_dbtp || limit_f.gain_db != 0.0f || limit_f.attack_ms != 0.0f || limit_f.release_ms != 0.0f))
    {
        fprintf(stderr, "zerovox: --limit-dbtp, --limit-gain-db, --limit-attack-ms and --limit-release-ms need --limit\n");
        usage(stderr);
        return 2;
    }
    if (resample_path.empty() ? rate_flag : !rate_flag || out_rate_flag)
    {
        fprintf(stderr, "zerovox: --resample IN.wav and --rate R need each other (--out-rate belongs to a synthesis run)\n");
        usage(stderr);
        return 2;
    }
    if (resample_path.empty() && !out_rate_flag && (resample_f.design || resample_f.dither || resample_f.seeded))
    {
        fprintf(stderr, "zerovox: --resample-zeros, --resample-beta, --resample-cutoff, --dither and --dither-seed need --resample IN.wav or --out-rate R\n");
        usage(stderr);
        return 2;
    }
    if ((!resample_path.empty() || out_rate_flag) &&
        (!limit_path.empty() || !loudness_path.empty() || !analyze_path.empty() || !align_a.empty() || planning || (!resample_path.empty() && !like_path.empty())))
    {
        fprintf(stderr, "zerovox: --resample IN.wav and --out-rate exclude --limit IN.wav, --loudness, --analyze, --align, --plan (and --resample excludes --time-like)\n");
        usage(stderr);
        return 2;
    }
    if (align_flag && align_a.empty())
    {
        fprintf(stderr, "zerovox: --mel-width, --align-scale, --align-normalise and --map-out need --align A.f32 B.f32\n");
        usage(stderr);
        return 2;
    }
    if (!align_a.empty() && !mel_width)
    {
        fprintf(stderr, "zerovox: --align needs --mel-width M\n");
        usage(stderr);
        return 2;
    }
    if (!like_path.empty() && (!align_a.empty() || !analyze_path.empty() || !pc_path.empty() || target_frames > 0 || target_seconds > 0.0))
    {
        fprintf(stderr, "zerovox: --time-like and --align, --analyze, --phoneme-controls, --target-frames, --target-seconds exclude each other\n");
        usage(stderr);
        return 2;
    }
    if (!band_hz.empty() && bands_path.empty() && pbands_path.empty())
    {
        fprintf(stderr, "zerovox: --band-edges-hz needs --bands FILE or --phoneme-bands FILE\n");
        usage(stderr);
        return 2;
    }
    if ((!eq_hz.empty() || eq_taps_given) && eq_db.empty())
    {
        fprintf(stderr, "zerovox: --eq-edges-hz and --eq-taps need --eq-gain-db\n");
        usage(stderr);
        return 2;
    }
    if (!taps_path.empty() && !eq_db.empty())
    {
        fprintf(stderr, "zerovox: --filter-taps and --eq-gain-db exclude each other\n");
        usage(stderr);
        return 2;
    }
    if (!eq_db.empty() && eq_db.size() != (eq_hz.empty() ? (size_t)16 : eq_hz.size() - 1))
    {
        fprintf(stderr, "zerovox: --eq-gain-db has %zu gains, %s gives %zu bands\n", eq_db.size(), eq_hz.empty() ? "the default" : "--eq-edges-hz",
                eq_hz.empty() ? (size_t)16 : eq_hz.size() - 1);
        usage(stderr);
        return 2;
    }
    std::vector<float> filter_taps;        // --filter-taps, read ahead of the checkpoint
    if (!taps_path.empty())
    {
        std::ifstream f(taps_path);
        std::string line;
        bool ok = (bool)f;
        while (ok && std::getline(f, line))
        {
            if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
            const size_t a0 = line.find_first_not_of(" \t\r"), a1 = line.find_last_not_of(" \t\r");
            const std::string item = line.substr(a0, a1 - a0 + 1);
            char *end = nullptr;
            const float x = strtof(item.c_str(), &end);
            ok = end == item.c_str() + item.size() && filter_taps.size() < 4096;
            filter_taps.push_back(x);
        }
        if (!ok || filter_taps.empty())
        {
            fprintf(stderr, "zerovox: --filter-taps: cannot read '%s' as one tap per line\n", taps_path.c_str());
            usage(stderr);
            return 2;
        }
    }
    if (pitch_param && pitch_path.empty() && ppitch_path.empty())
    {
        fprintf(stderr, "zerovox: --pitch-min-hz, --pitch-max-hz and --pitch-threshold need --pitch FILE or --phoneme-pitch FILE\n");
        usage(stderr);
        return 2;
    }

    try
    {
        if (info)
        {
            uint32_t n_tensors = 0, max_seq_len = 0;
            if (zv_gguf_inspect(model_path.c_str(), &n_tensors, &max_seq_len, -1, nullptr, nullptr, nullptr) != ZV_OK)
                throw std::runtime_error(zv_last_error());
            printf("%s: %u tensors, max_seq_len %u\n", model_path.c_str(), n_tensors, max_seq_len);
            for (uint32_t i = 0; i < n_tensors; i++)
            {
                char name[64];
                uint32_t type = 0;
                int64_t ne[4];
                if (zv_gguf_inspect(model_path.c_str(), nullptr, nullptr, (int)i, name, &type, ne) != ZV_OK)
                    throw std::runtime_error(zv_last_error());
                printf("  %-48s %s [%lld, %lld, %lld, %lld]\n", name, type == 0 ? "f32" : (type == 1 ? "f16" : "other"),
                       (long long)ne[0], (long long)ne[1], (long long)ne[2], (long long)ne[3]);
            }
            return 0;
        }

        if (planning) return plan(model_path, utt_path, controlled ? &prosody : nullptr);
        if (!analyze_path.empty()) return analyze(model_path, analyze_path, melout_path, resynth_path, mel_q);
        if (!loudness_path.empty()) return loudness_file(model_path, loudness_path, loud_q);
        if (!limit_path.empty()) return limit_file(model_path, limit_path, out_path, limit_f);
        if (!resample_path.empty()) return resample_file(model_path, resample_path, out_path, resample_f);
        if (!align_a.empty()) return align_files(model_path, align_a, align_b, (uint32_t)mel_width, align_q, map_path);
        std::vector<float> like_wav;                            // --time-like, read ahead of the checkpoint
        uint32_t like_rate = 0;
        if (!like_path.empty()) like_wav = read_pcm16("--time-like", like_path, like_rate);

        // per-phoneme controls and timings: the file is checked against the utterance before the model is loaded
        std::vector<int32_t> ids0;
        PhonemeControlFile pcf;
        std::vector<float> gains;
        if (!pc_path.empty() || !align_path.empty() || !gain_path.empty()) ids0 = utterance_ids(utt_path);
        if (!pc_path.empty()) pcf = read_phoneme_controls(pc_path, ids0.size());
        if (!gain_path.empty()) gains = read_phoneme_gains(gain_path, ids0.size());

        ZeroVOX::ZeroVOXModel model(model_path);
        const ZeroVOX::zerovox_hparams &hp = model.get_hparams();
        if (controlled) model.set_prosody(prosody);
        if (fit) model.set_fitted(true);
        if (leveled) model.set_volume(volume);
        if (enveloped)
        {
            // 600 000 ms at any rate below 3.5 MHz stay under the 0x7fffffff samples a fade may have
            const double rate = hp.audio_sampling_rate;
            const zv_envelope env = {gains.empty() ? nullptr : gains.data(), (uint32_t)ramp_frames,
                                     (uint32_t)std::min(floor(fade_ms[0] * rate / 1000.0 + 0.5), 2147483647.0),
                                     (uint32_t)std::min(floor(fade_ms[1] * rate / 1000.0 + 0.5), 2147483647.0)};
            model.set_envelope(&env, (uint32_t)gains.size());
        }
        if (!contour_path.empty() || !plevel_path.empty()) model.set_contour(!contour_path.empty(), !plevel_path.empty());
        if (!pitch_path.empty() || !ppitch_path.empty())
        {
            // Hz to lags on the host: the shortest lag is the highest frequency's period, truncated
            const double rate = hp.audio_sampling_rate;
            const zv_pitch pit = {nullptr, nullptr, pitch_hz[1] > 0.0 ? (uint32_t)std::min(floor(rate / pitch_hz[1]), 4294967295.0) : 0u,
                                  pitch_hz[0] > 0.0 ? (uint32_t)std::min(floor(rate / pitch_hz[0]), 4294967295.0) : 0u, 0u, (float)pitch_thr};
            model.set_pitch(!pitch_path.empty(), !ppitch_path.empty(), &pit);
        }
        std::vector<uint32_t> band_edges;      // the bins in force, for the TSV headers
        if (!bands_path.empty() || !pbands_path.empty())
        {
            // Hz to bins on the host: round(hz * 1024 / rate)
            for (double hz : band_hz) band_edges.push_back((uint32_t)std::min(floor(hz * 1024.0 / hp.audio_sampling_rate + 0.5), 4294967295.0));
            for (size_t b = 1; b < band_edges.size(); b++)
                if (band_edges[b] <= band_edges[b - 1])
                    throw std::runtime_error("--band-edges-hz: " + std::to_string(band_hz[b - 1]) + " and " + std::to_string(band_hz[b]) +
                                             " Hz fall on the same bin " + std::to_string(band_edges[b]) + " at " +
                                             std::to_string(hp.audio_sampling_rate) + " Hz");
            model.set_bands(!bands_path.empty(), !pbands_path.empty(), band_edges.empty() ? 0u : (uint32_t)band_edges.size() - 1,
                            band_edges.empty() ? nullptr : band_edges.data());
            band_edges = model.get_band_edges();       // the library's defaults where none were given
        }
        if (!filter_taps.empty()) model.set_filter(filter_taps.data(), (uint32_t)filter_taps.size());
        if (!eq_db.empty())
        {
            // Hz to bins as for --band-edges-hz, dB to linear gains, then the library's design
            std::vector<uint32_t> eq_edges;
            for (double hz : eq_hz) eq_edges.push_back((uint32_t)std::min(floor(hz * 1024.0 / hp.audio_sampling_rate + 0.5), 4294967295.0));
            for (size_t b = 1; b < eq_edges.size(); b++)
                if (eq_edges[b] <= eq_edges[b - 1])
                    throw std::runtime_error("--eq-edges-hz: " + std::to_string(eq_hz[b - 1]) + " and " + std::to_string(eq_hz[b]) +
                                             " Hz fall on the same bin " + std::to_string(eq_edges[b]) + " at " +
                                             std::to_string(hp.audio_sampling_rate) + " Hz");
            std::vector<float> g;
            for (double db : eq_db) g.push_back((float)pow(10.0, db / 20.0));
            std::vector<float> taps((size_t)eq_taps);
            if (zv_filter_design(eq_edges.empty() ? 0u : (uint32_t)eq_edges.size() - 1, eq_edges.empty() ? nullptr : eq_edges.data(), g.data(),
                                 (uint32_t)eq_taps, taps.data()) != ZV_OK)
                throw std::runtime_error(zv_last_error());
            model.set_filter(taps.data(), (uint32_t)taps.size());
        }
        if (target_seconds > 0.0)
            target_frames = (long)std::min(floor(target_seconds * hp.audio_sampling_rate / hp.audio_hop_size + 0.5), 1e9);
        if (target_frames > 0 || target_seconds > 0.0)
        {
            // the capacity of every eval() is the checkpoint's max_seq_len
            if (target_frames < 1 || target_frames > (long)hp.max_seq_len)
            {
                fprintf(stderr, "zerovox: a target of %ld frames is outside [1, %u], the checkpoint's max_seq_len\n", target_frames,
                        hp.max_seq_len);
                usage(stderr);
                return 2;
            }
            model.set_target_frames((uint32_t)target_frames);
        }
        if (!pc_path.empty())
        {
            const zv_phoneme_controls pc = {pcf.frames.data(), pcf.scale.data(), pcf.pitch.data(), pcf.energy.data()};
            model.set_phoneme_controls(&pc, (uint32_t)ids0.size());
        }
        else if (!align_path.empty())
            model.set_phoneme_controls(nullptr, (uint32_t)ids0.size());        // timings only
        if (!like_path.empty())
        {
            if (like_rate != hp.audio_sampling_rate)
                throw std::runtime_error("--time-like: '" + like_path + "' is at " + std::to_string(like_rate) + " Hz, the model at " +
                                         std::to_string(hp.audio_sampling_rate) + " Hz (nothing is resampled)");
            model.set_time_like(like_wav.data(), like_wav.size());
            fit = true;                                         // the reference's whole hops are what is written
        }
        if (utt_path.empty())
            model.eval();
        else
        {
            std::ifstream f(utt_path);
            if (!f) throw std::runtime_error("cannot open utterance file '" + utt_path + "'");
            std::string l1, l2, l3;
            if (!std::getline(f, l1) || !std::getline(f, l2) || !std::getline(f, l3))
                throw std::runtime_error("utterance file needs three lines (ids, punctuation ids, style)");
            std::vector<int32_t> ids = parse_line<int32_t>(l1), puncts = parse_line<int32_t>(l2);
            std::vector<float> style = parse_line<float>(l3);
            const size_t E = hp.emb_dim + hp.punct_emb_dim;
            if (ids.empty() || ids.size() != puncts.size())
                throw std::runtime_error("utterance file: need as many punctuation ids as phoneme ids (> 0)");
            if (style.size() == 1 && style[0] == 0.0f) style.assign(E, 0.0f);
            if (style.size() != E)
                throw std::runtime_error("utterance file: style vector has " + std::to_string(style.size()) + " values, model needs " +
                                         std::to_string(E));
            model.eval(ids.data(), puncts.data(), style.data(), (uint32_t)ids.size());
        }

        const uint32_t nf = model.get_num_frames();
        if (!like_path.empty())
        {
            const zv_alignment &al = model.get_alignment();
            printf("time-like: %u frames, alignment total %llu path_len %u distance %.9g\n", nf, (unsigned long long)al.total, al.path_len, al.distance);
        }
        if (leveled)
        {
            const zv_level &lv = model.get_level();
            printf("level: rms %.9g peak %.9g gain %.9g\n", (double)lv.rms, (double)lv.peak, (double)lv.gain);
        }
        if (!align_path.empty())
        {
            FILE *af = fopen(align_path.c_str(), "w");
            if (!af) throw std::runtime_error("cannot open '" + align_path + "' for writing");
            const std::vector<int32_t> &dur = model.get_durations();
            fprintf(af, "index\tphoneme_id\tstart_frame\tframes\tstart_sample\tsamples\n");
            uint64_t start = 0;
            for (size_t i = 0; i < dur.size() && i < ids0.size(); i++)
            {
                fprintf(af, "%zu\t%d\t%llu\t%d\t%llu\t%llu\n", i, ids0[i], (unsigned long long)start, dur[i],
                        (unsigned long long)(start * hp.audio_hop_size), (unsigned long long)dur[i] * hp.audio_hop_size);
                start += (uint64_t)dur[i];
            }
            if (fclose(af) != 0) throw std::runtime_error("short write to '" + align_path + "'");
        }
        // the contour's tables: %.9g prints an f32 so that it reads back to the same bits
        auto write_levels = [](const std::string &path, const std::vector<zv_frame_level> &rows) {
            FILE *cf = fopen(path.c_str(), "w");
            if (!cf) throw std::runtime_error("cannot open '" + path + "' for writing");
            fprintf(cf, "index\trms\tpeak\n");
            for (size_t i = 0; i < rows.size(); i++) fprintf(cf, "%zu\t%.9g\t%.9g\n", i, (double)rows[i].rms, (double)rows[i].peak);
            if (fclose(cf) != 0) throw std::runtime_error("short write to '" + path + "'");
        };
        if (!contour_path.empty()) write_levels(contour_path, model.get_frame_levels());
        if (!plevel_path.empty()) write_levels(plevel_path, model.get_phoneme_levels());
        if (!pitch_path.empty() || !ppitch_path.empty())
        {
            auto write_pitch = [](const std::string &path, const char *last, size_t rows, const float *ab) {
                FILE *cf = fopen(path.c_str(), "w");
                if (!cf) throw std::runtime_error("cannot open '" + path + "' for writing");
                fprintf(cf, "index\tf0_hz\t%s\n", last);
                for (size_t i = 0; i < rows; i++) fprintf(cf, "%zu\t%.9g\t%.9g\n", i, (double)ab[2 * i], (double)ab[2 * i + 1]);
                if (fclose(cf) != 0) throw std::runtime_error("short write to '" + path + "'");
            };
            static_assert(sizeof(zv_pitch_frame) == 8 && sizeof(zv_pitch_phoneme) == 8, "two floats per row");
            if (!pitch_path.empty()) write_pitch(pitch_path, "strength", model.get_pitch_frames().size(), &model.get_pitch_frames().data()->f0_hz);
            if (!ppitch_path.empty())
                write_pitch(ppitch_path, "voiced", model.get_pitch_phonemes().size(), &model.get_pitch_phonemes().data()->f0_hz);
        }
        if (!bands_path.empty() || !pbands_path.empty())
        {
            auto write_bands = [&](const std::string &path, const std::vector<float> &rows) {
                FILE *cf = fopen(path.c_str(), "w");
                if (!cf) throw std::runtime_error("cannot open '" + path + "' for writing");
                const size_t nb = band_edges.size() - 1;
                fprintf(cf, "index");
                for (size_t b = 0; b < nb; b++) fprintf(cf, "\t%u-%u", band_edges[b], band_edges[b + 1]);
                fprintf(cf, "\n");
                for (size_t i = 0; i < rows.size() / nb; i++)
                {
                    fprintf(cf, "%zu", i);
                    for (size_t b = 0; b < nb; b++) fprintf(cf, "\t%.9g", (double)rows[i * nb + b]);
                    fprintf(cf, "\n");
                }
                if (fclose(cf) != 0) throw std::runtime_error("short write to '" + path + "'");
            };
            if (!bands_path.empty()) write_bands(bands_path, model.get_band_frames());
            if (!pbands_path.empty()) write_bands(pbands_path, model.get_band_phonemes());
        }
        // --out-rate R: what -o would receive goes through zv_resample_wave and is written at R Hz from the device's int16 samples
        auto write_at_out_rate = [&](const float *data, size_t n) {
            if (!out_rate_flag) return false;
            resample_to_file("resample", n, resample_ask(resample_f, hp.audio_sampling_rate), out_path,
                             [&](const zv_resample &q, int16_t *out) { return model.resample(data, n, &q, nullptr, out); });
            return true;
        };
        if (loud_q.flags)
        {
            // --lufs / --true-peak-dbtp: what -o receives, measured over the speech and scaled as a whole, then written
            const uint32_t T = trim || fit ? nf : hp.max_seq_len;
            std::vector<float> scaled((size_t)T * hp.audio_hop_size);
            zv_loudness_result r{};
            if (limit && T)
            {
                // --limit: the gain of the target alone, then the limiter under the ceiling, then the meter on what is written
                const zv_loudness target = {loud_q.gain, loud_q.target_lufs, 0.0f, ZV_LOUDNESS_TARGET};
                r = model.loudness(model.get_wav(), T, std::min(nf, T), &target, nullptr);
                const zv_limiter lq = limit_ask(limit_f, hp.audio_sampling_rate, r.gain, loud_q.true_peak_ceiling);
                const zv_limit_result lr = model.limit(model.get_wav(), T, std::min(nf, T), &lq, scaled.data());
                print_loudness("loudness before the gain", r);
                print_limit("limiter", lr);
                print_loudness("loudness after the limiter", model.loudness(scaled.data(), T, std::min(nf, T), nullptr, nullptr));
            }
            else
            {
                if (T) r = model.loudness(model.get_wav(), T, std::min(nf, T), &loud_q, scaled.data());
                print_loudness("loudness before the gain", r);
            }
            if (write_at_out_rate(scaled.data(), scaled.size())) return 0;
            if (zv_write_wav(out_path.c_str(), scaled.data(), scaled.size(), hp.audio_sampling_rate) != ZV_OK) throw std::runtime_error(zv_last_error());
            printf("Successfully created %s with %zu samples (%u frames).\n", out_path.c_str(), scaled.size(), T);
        }
        else if (trim || fit)
        {
            const size_t n = (size_t)nf * hp.audio_hop_size;
            if (write_at_out_rate(model.get_wav(), n)) return 0;
            if (zv_write_wav(out_path.c_str(), model.get_wav(), n, hp.audio_sampling_rate) != ZV_OK)
                throw std::runtime_error(zv_last_error());
            printf("Successfully created %s with %zu samples (%u frames).\n", out_path.c_str(), n, nf);
        }
        else
        {
            if (write_at_out_rate(model.get_wav(), (size_t)hp.max_seq_len * hp.audio_hop_size)) return 0;
            if (!model.write_wav_file(out_path)) throw std::runtime_error(zv_last_error());
            printf("Successfully created %s with %zu samples.\n", out_path.c_str(), (size_t)hp.max_seq_len * hp.audio_hop_size);
        }
    }
    catch (const std::exception &e)
    {
        fprintf(stderr, "zerovox: %s\n", e.what());
        return 1;
    }
    return 0;
}

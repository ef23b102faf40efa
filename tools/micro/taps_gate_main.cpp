// Replays the refusal corpus of the tap-table gate (tests/taps_gate.py: refusal_corpus) against vnd_taps_create and
// vnd_taps_deserialize, from a file tools/taps_gate_sanitize.py wrote.  Built with the host sanitizers and linked against
// a library built the same way: a stand-alone program, CPU only - every case is refused before the gate would touch the
// context, which is a pointer that must never be followed.
//
// File: int32 words.  "VNDG", case count, then per case
//   create: 0, status, null_out, null_ctx, C, apply_gain, then 7 arrays (tap_offsets, tap_index, tap_weight, seg_offsets,
//           seg_end, seg_gain, chan_flags): present, bytes, the bytes padded to whole words
//   image:  1, status, null_out, null_ctx, misaligned, has_buffer, nbytes (as passed; may lie), bytes held, the bytes padded
// Every array is copied into a heap block of exactly its size, so that a read past it is the sanitizer's to see.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vnd_amd.h"

namespace {

struct Block {                                   // an exact-size heap copy (nullptr when absent)
    void *p = nullptr;
    Block(const int32_t *words, int32_t bytes, bool present, int shift = 0)
    {
        if (!present) return;
        base = (char *)malloc((size_t)bytes + (size_t)shift + (bytes + shift == 0 ? 1 : 0));
        if (bytes) memcpy(base + shift, words, (size_t)bytes);
        p = base + shift;
    }
    ~Block() { free(base); }
    Block(const Block &) = delete;
    char *base = nullptr;
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s corpus-file\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<int32_t> w;
    int32_t buf[4096];
    for (size_t got; (got = fread(buf, 4, 4096, f)) > 0;) w.insert(w.end(), buf, buf + got);
    fclose(f);
    if (w.size() < 2 || w[0] != 0x474e4456) { fprintf(stderr, "not a corpus file\n"); return 2; }
    vnd_ctx *fake = (vnd_ctx *)0x1000;
    size_t at = 2;
    int failures = 0;
    for (int32_t n = 0; n < w[1]; ++n) {
        const int32_t kind = w[at], want = w[at + 1], null_out = w[at + 2], null_ctx = w[at + 3];
        vnd_taps *taps = (vnd_taps *)0xdead;
        vnd_status st;
        if (kind == 0) {
            const int32_t C = w[at + 4], gain = w[at + 5];
            at += 6;
            const int32_t *data[7];
            int32_t bytes[7], present[7];
            for (int a = 0; a < 7; ++a) {
                present[a] = w[at]; bytes[a] = w[at + 1]; data[a] = w.data() + at + 2;
                at += 2 + (size_t)(bytes[a] + 3) / 4;
            }
            Block off(data[0], bytes[0], present[0]), idx(data[1], bytes[1], present[1]), wt(data[2], bytes[2], present[2]),
                so(data[3], bytes[3], present[3]), se(data[4], bytes[4], present[4]), sg(data[5], bytes[5], present[5]),
                fl(data[6], bytes[6], present[6]);
            st = vnd_taps_create(null_ctx ? nullptr : fake, C, (const int32_t *)off.p, (const int32_t *)idx.p, (const float *)wt.p,
                                 (const int32_t *)so.p, (const int32_t *)se.p, (const float *)sg.p, (const uint8_t *)fl.p, gain,
                                 null_out ? nullptr : &taps);
        } else {
            const int32_t misaligned = w[at + 4], has_buffer = w[at + 5], nbytes = w[at + 6], held = w[at + 7];
            Block image(w.data() + at + 8, held, has_buffer != 0, misaligned ? 1 : 0);
            at += 8 + (size_t)(held + 3) / 4;
            st = vnd_taps_deserialize(null_ctx ? nullptr : fake, image.p, nbytes, null_out ? nullptr : &taps);
        }
        const char *msg = vnd_last_error();
        if ((int32_t)st != want || !msg || !*msg || (!null_out && taps != nullptr)) {
            fprintf(stderr, "case %d (%s): status %d, expected %d; message \"%s\"; *taps %p\n", n, kind ? "image" : "create",
                    (int)st, want, msg ? msg : "", (void *)taps);
            ++failures;
        }
    }
    printf("taps_gate_main: %d cases replayed, %d failed\n", w[1], failures);
    return failures ? 1 : 0;
}

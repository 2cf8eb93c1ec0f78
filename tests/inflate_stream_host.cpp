// The stream inflate of csrc/bdx_inflate_stream_core.h compiled as plain C++: every kernel of csrc/bdx_inflate_stream.hip
// is a loop over its workgroups here, in the order of the launches.  tests/test_device_gunzip_stream_cpu.py loads it as
// a library and holds it to the cases of tests/inflate_stream_cases.py; with -DINFS_HOST_MAIN it is the stand-alone
// driver that tests/test_device_gunzip_stream_sanitize.py runs under AddressSanitizer.  The file, the staging image
// and the output are exact-size heap blocks: one byte beside any of them is the sanitizer's to report.
// infs_host_set_launch makes the loops start their workgroups as the device does (tests/test_device_gunzip_stream_fuzz_cpu.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../biodemux.jl_amd/csrc/bdx_inflate_stream_core.h"

static InfsShared X;

// How the device starts a kernel.  fill < 0: X is the one zero-initialised object of the program, carried through every
// item, kernel and call, with inf_ph_tables at the top of a call.  fill in 0 .. 255: every workgroup begins with X full of
// that byte (the LDS holds whatever the workgroup before left there) and runs what its kernel of
// csrc/bdx_inflate_stream.hip runs in front of its loop; a grid of `grid` workgroups deals the items b, b + grid, ...
// to workgroup b on that one X (grid 0: a workgroup per item).
static int g_fill = -1;
static int64_t g_grid = 0;
extern "C" void infs_host_set_launch(int fill, int grid) {
    g_fill = fill < 0 ? -1 : fill & 255;
    g_grid = grid > 0 ? grid : 0;
}
static int64_t wg_count(int64_t n) { return g_fill >= 0 && g_grid > 0 && g_grid < n ? g_grid : n; }
static void wg_begin(bool tables) {
    if (g_fill < 0) return;
    memset(&X, g_fill, sizeof X);
    if (tables) INF_PHASE(inf_ph_tables(X.S, t))
}

extern "C" int32_t infs_host_chunk_default(void) { return INFS_CHUNK_DEFAULT; }
extern "C" int32_t infs_host_shared_bytes(void) { return (int32_t)sizeof(InfsShared); }

// comp[0, comp_len) -> out[0, *plain_len).  Returns 0, a status INF_E_* (member and at say where), or -5 when out_cap
// is too small (*plain_len is what is needed; out is untouched).  seg_room: the first room of the segment list (a
// small one makes the chain run twice).
extern "C" int32_t infs_host_inflate(const uint8_t *comp_in, int64_t comp_len, int32_t chunk, uint8_t *out_user, int64_t out_cap,
                                     int64_t *plain_len, int64_t *info, int32_t *member, int64_t *at, int64_t seg_room) {
    if (chunk == 0) chunk = INFS_CHUNK_DEFAULT;
    if (g_fill < 0) INF_PHASE(inf_ph_tables(X.S, t))
    uint8_t *comp = (uint8_t *)malloc(comp_len > 0 ? (size_t)comp_len : 1);
    if (comp_len > 0) memcpy(comp, comp_in, (size_t)comp_len);
    const int64_t n_chunks = (comp_len + chunk - 1) / chunk;
    std::vector<InfsRecord> rec((size_t)n_chunks + 1);
    for (int64_t b = 0, wgs = wg_count(n_chunks); b < wgs; ++b) {  // infs_scan_kernel: tables, then its chunks
        wg_begin(true);
        for (int64_t k = b; k < n_chunks; k += wgs) infs_scan_chunk(X, comp, comp_len, chunk, k, &rec[(size_t)k]);
    }
    std::vector<InfsSegment> seg((size_t)(seg_room > 0 ? seg_room : 1));
    InfsResult res;
    memset(&res, 0, sizeof res);
    wg_begin(true);  // infs_chain_kernel: one workgroup, tables
    infs_chain(X, comp, comp_len, chunk, rec.data(), n_chunks, seg.data(), (int64_t)seg.size(), &res);
    if (res.status == INF_OK && res.n_seg > seg.size()) {
        seg.resize((size_t)res.n_seg);
        wg_begin(true);  // infs_chain_kernel again, with the room it asked for
        infs_chain(X, comp, comp_len, chunk, rec.data(), n_chunks, seg.data(), (int64_t)seg.size(), &res);
    }
    int32_t rc = (int32_t)res.status;
    if (rc == INF_OK) {
        *plain_len = (int64_t)res.total;
        if (info) memcpy(info, res.info, sizeof res.info);
        if ((int64_t)res.total > out_cap) rc = -5;
    }
    if (rc == INF_OK) {
        const int64_t n_seg = (int64_t)res.n_seg;
        uint16_t *stage = (uint16_t *)malloc(res.total ? (size_t)res.total * 2 : 2);
        uint8_t *out = (uint8_t *)malloc(res.total ? (size_t)res.total : 1);
        for (int64_t b = 0, wgs = wg_count(n_seg); b < wgs; ++b) {  // infs_decode_kernel: NO tables, its segments
            wg_begin(false);
            for (int64_t i = b; i < n_seg; i += wgs) infs_decode_segment(X, comp, comp_len, &seg[(size_t)i], stage);
        }
        wg_begin(false);  // infs_tails_kernel: one workgroup that has no shared state at all
        infs_tails(seg.data(), n_seg, stage, out);
        for (int64_t b = 0, wgs = wg_count(n_seg); b < wgs; ++b) {  // infs_rest_kernel: tables, then its segments
            wg_begin(true);
            for (int64_t i = b; i < n_seg; i += wgs) infs_rest_segment(X, &seg[(size_t)i], stage, out);
        }
        wg_begin(true);  // infs_verdict_kernel: one workgroup, tables
        INF_PHASE(infs_ph_verdict(X, seg.data(), n_seg, &res, t))
        rc = (int32_t)res.status;
        if (rc == INF_OK && res.total) memcpy(out_user, out, (size_t)res.total);
        free(out);
        free(stage);
    }
    if (rc > 0) {
        if (member) *member = (int32_t)res.member;
        if (at) *at = (int64_t)res.at;
    }
    free(comp);
    return rc;
}

#ifdef INFS_HOST_MAIN
static std::vector<uint8_t> slurp(const std::string &path) {
    std::vector<uint8_t> all;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path.c_str());
        exit(3);
    }
    uint8_t buf[65536];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + got);
    fclose(f);
    return all;
}

// exact sizes again: the output is exactly as large as the plain text
static int32_t run(const std::vector<uint8_t> &comp, size_t clen, int32_t chunk, size_t cap, std::vector<uint8_t> *got, size_t *need = nullptr) {
    uint8_t *in = (uint8_t *)malloc(clen ? clen : 1);
    uint8_t *out = (uint8_t *)malloc(cap ? cap : 1);
    if (clen) memcpy(in, comp.data(), clen);
    int64_t plen = 0;
    const int32_t st = infs_host_inflate(in, (int64_t)clen, chunk, out, (int64_t)cap, &plen, nullptr, nullptr, nullptr, 3);
    if (got) got->assign(out, out + (st == 0 ? (size_t)plen : 0));
    if (need) *need = (size_t)plen;
    free(out);
    free(in);
    return st;
}

// <dir> <cases> [<fill> <grid>]: case_K.gz, case_K.plain, case_K.info ("<1: good, + 2: as it is only> <chunk> <chunk> ...")
int main(int argc, char **argv) {
    if (argc != 3 && argc != 5) return 2;
    if (argc == 5) infs_host_set_launch(atoi(argv[3]), atoi(argv[4]));
    const std::string dir = argv[1];
    const int cases = atoi(argv[2]);
    long good = 0, bad = 0, cut = 0, mangled = 0;
    uint64_t rng = 88172645463325252ull;
    for (int k = 0; k < cases; ++k) {
        const std::string stem = dir + "/case_" + std::to_string(k);
        const std::vector<uint8_t> comp = slurp(stem + ".gz"), want = slurp(stem + ".plain"), info = slurp(stem + ".info");
        std::vector<int> words;
        std::string line(info.begin(), info.end());
        for (char *p = strtok(&line[0], " \n"); p; p = strtok(nullptr, " \n")) words.push_back(atoi(p));
        if (words.size() < 2) return 4;
        const bool is_good = words[0] & 1, as_it_is = words[0] & 2;
        const size_t room = is_good ? want.size() : (size_t)1 << 17;  // (a bad one: room to get to its fault)
        for (size_t c = 1; c < words.size(); ++c) {
            std::vector<uint8_t> got;
            size_t need = 0;
            int32_t st = run(comp, comp.size(), words[c], room, &got, &need);
            if (!is_good && st == -5 && need > room) st = run(comp, comp.size(), words[c], need, &got);  // (its fault is in its bytes, not its blocks)
            if (is_good ? (st != 0 || got != want) : st <= 0) {
                fprintf(stderr, "case %d chunk %d: status %d\n", k, words[c], st);
                return 5;
            }
        }
        (is_good ? good : bad)++;
        if (comp.size() > 1500 || as_it_is) continue;
        for (size_t c = 0; c < comp.size(); ++c, ++cut) (void)run(comp, c, 64, room, nullptr);  // every prefix
        for (int r = 0; r < 150; ++r, ++mangled) {  // corrupted bytes anywhere; outputs too small and too large
            std::vector<uint8_t> c = comp;
            for (int j = 0; j < 1 + r % 3; ++j) {
                rng ^= rng << 13;
                rng ^= rng >> 7;
                rng ^= rng << 17;
                c[rng % c.size()] ^= (uint8_t)(1u << ((rng >> 32) & 7));
            }
            const size_t cap = r % 5 == 0 ? room / 2 : r % 7 == 0 ? room + 100 : room;
            (void)run(c, c.size(), r % 2 ? 64 : 256, cap, nullptr);
        }
    }
    printf("stream inflate driver ok: %ld good, %ld bad, %ld cut, %ld mangled\n", good, bad, cut, mangled);
    return 0;
}
#endif

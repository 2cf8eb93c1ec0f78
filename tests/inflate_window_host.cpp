// The windowed stream inflate of csrc/bdx_inflate_window_core.h compiled as plain C++: every kernel that
// bdx_fq_inflate_window_feed launches is a loop over its workgroups here, in the order of the launches.  It includes
// tests/inflate_stream_host.cpp: the whole-file build is in the same library (the yardstick for refusals), and its launch
// emulation (infs_host_set_launch: every workgroup starts from a state full of a fill byte, a grid deals the items) is
// the one used here.  The carried state, the window's bytes, the staging image and the output are exact-size heap
// blocks.  tests/test_device_gunzip_window_cpu.py loads it as a library; with -DINFW_HOST_MAIN it is the stand-alone
// driver that tests/test_device_gunzip_window_sanitize.py runs under AddressSanitizer.
#include "inflate_stream_host.cpp"

#include "../biodemux.jl_amd/csrc/bdx_inflate_window_core.h"

static InfwShared W;  // the chain's workgroup

struct InfwHost {
    InfwCarry *carry;
    int dead;
};

extern "C" int32_t infw_host_shared_bytes(void) { return (int32_t)sizeof(InfwShared); }
extern "C" void *infw_host_open(void) {
    InfwHost *h = new InfwHost;
    h->carry = (InfwCarry *)calloc(1, sizeof(InfwCarry));
    h->dead = 0;
    return h;
}
extern "C" void infw_host_close(void *hv) {
    InfwHost *h = (InfwHost *)hv;
    if (!h) return;
    free(h->carry);
    delete h;
}
// where, bit, member, member_n, comp_abs, plain_abs of the carried state
extern "C" void infw_host_state(void *hv, int64_t *six) {
    const InfwCarry *C = ((InfwHost *)hv)->carry;
    six[0] = C->where, six[1] = C->bit, six[2] = C->member, six[3] = (int64_t)C->member_n, six[4] = (int64_t)C->comp_abs, six[5] = (int64_t)C->plain_abs;
}

static void chain_begin() {
    if (g_fill >= 0) memset(&W, g_fill, sizeof W);
    INF_PHASE(inf_ph_tables(W.X.S, t))
}

// One bdx_fq_inflate_window_feed.  Returns 0, a status INF_E_* (member and at say where; the object is dead), -5 when
// out_cap is too small (*plain_len is the room needed; out and the carried state are untouched), -3 on a dead object.
extern "C" int32_t infw_host_feed(void *hv, const uint8_t *comp_in, int64_t comp_len, int32_t last, int32_t chunk, uint8_t *out_user,
                                  int64_t out_cap, int64_t *consumed, int64_t *plain_len, int64_t *info, int32_t *member, int64_t *at,
                                  int64_t seg_room) {
    InfwHost *h = (InfwHost *)hv;
    *consumed = *plain_len = 0;
    if (h->dead) return -3;
    InfwCarry *C = h->carry;
    if (C->where == INFW_IGNORE) {
        *consumed = comp_len;
        return 0;
    }
    if (chunk == 0) chunk = INFS_CHUNK_DEFAULT;
    if (g_fill < 0) INF_PHASE(inf_ph_tables(X.S, t))
    uint8_t *comp = (uint8_t *)malloc(comp_len > 0 ? (size_t)comp_len : 1);
    if (comp_len > 0) memcpy(comp, comp_in, (size_t)comp_len);
    const int64_t n_chunks = (comp_len + chunk - 1) / chunk;
    std::vector<InfsRecord> rec((size_t)n_chunks + 1);
    for (int64_t b = 0, wgs = wg_count(n_chunks); b < wgs; ++b) {  // infw_scan_kernel: tables, then its chunks
        wg_begin(true);
        for (int64_t k = b; k < n_chunks; k += wgs) infw_scan_chunk(X, comp, comp_len, chunk, k, C, &rec[(size_t)k]);
    }
    std::vector<InfsSegment> seg((size_t)(seg_room > 0 ? seg_room : 1));
    InfwResult res;
    memset(&res, 0, sizeof res);
    chain_begin();  // infw_chain_kernel: one workgroup, tables
    infw_chain(W, comp, comp_len, last, chunk, rec.data(), n_chunks, seg.data(), (int64_t)seg.size(), C, &res);
    if (res.r.status == INF_OK && res.r.n_seg > seg.size()) {
        seg.resize((size_t)res.r.n_seg);
        chain_begin();
        infw_chain(W, comp, comp_len, last, chunk, rec.data(), n_chunks, seg.data(), (int64_t)seg.size(), C, &res);
    }
    int32_t rc = (int32_t)res.r.status;
    if (rc == INF_OK) {
        *plain_len = (int64_t)res.r.total;
        if (info) memcpy(info, res.r.info, sizeof res.r.info);
        if ((int64_t)res.r.total > out_cap) rc = -5;
    }
    if (rc == INF_OK) {
        const int64_t n_seg = (int64_t)res.r.n_seg;
        const uint64_t total = res.r.total;
        uint16_t *stage = (uint16_t *)malloc(total ? (size_t)total * 2 : 2);
        uint8_t *out = (uint8_t *)malloc(total ? (size_t)total : 1);
        const uint8_t *hist = C->hist[C->cur & 1];
        if (n_seg > 0) {
            for (int64_t b = 0, wgs = wg_count(n_seg); b < wgs; ++b) {  // infs_decode_kernel: NO tables
                wg_begin(false);
                for (int64_t i = b; i < n_seg; i += wgs) infs_decode_segment(X, comp, comp_len, &seg[(size_t)i], stage);
            }
            wg_begin(false);  // infs_tails_kernel
            infs_tails(seg.data(), n_seg, stage, out, hist);
            for (int64_t b = 0, wgs = wg_count(n_seg); b < wgs; ++b) {  // infs_rest_kernel: tables
                wg_begin(true);
                for (int64_t i = b; i < n_seg; i += wgs) infs_rest_segment(X, &seg[(size_t)i], stage, out, hist);
            }
        }
        wg_begin(true);  // infw_verdict_kernel: one workgroup, tables
        infw_verdict(X, seg.data(), n_seg, out, total, C, &res);
        rc = (int32_t)res.r.status;
        if (rc == INF_OK) {
            if (total) memcpy(out_user, out, (size_t)total);
            *consumed = (int64_t)res.consumed;
        }
        free(out);
        free(stage);
    }
    if (rc > 0) {
        h->dead = 1;
        if (member) *member = (int32_t)res.r.member;
        if (at) *at = (int64_t)res.r.at;
    }
    free(comp);
    return rc;
}

// A whole file through one object under a schedule: window i offers sizes[i] bytes (behind the list: all that is left);
// a window without progress is offered again, twice as long.  Every window's output is an exact-size block: the first
// call is made without room and says what is needed.  -> 0 and out[0, *plain_len), or the refusal; -5 when out_cap is
// too small; -9 when a call breaks its contract (for the caller to report).
extern "C" int32_t infw_host_run(const uint8_t *comp, int64_t len, const int64_t *sizes, int64_t n_sizes, int32_t chunk, uint8_t *out, int64_t out_cap,
                                 int64_t *plain_len, int32_t *member, int64_t *at, int64_t *windows, int64_t seg_room) {
    void *h = infw_host_open();
    int64_t pos = 0, total = 0, i = 0, n_win = 0, grow = 0;
    int32_t rc = 0;
    for (;;) {
        int64_t want = grow ? grow : i < n_sizes ? sizes[i] : len - pos;
        if (want > len - pos) want = len - pos;
        const int32_t last = pos + want == len;
        int64_t used = 0, plen = 0, need = 0;
        uint8_t *win = (uint8_t *)malloc(want ? (size_t)want : 1);
        if (want) memcpy(win, comp + pos, (size_t)want);
        uint8_t none = 0x5A;
        rc = infw_host_feed(h, win, want, last, chunk, &none, 0, &used, &need, nullptr, member, at, seg_room);
        uint8_t *o = nullptr;
        if (rc == 0 && need != 0) rc = -9;
        if (rc == -5) {
            if (none != 0x5A || used != 0 || need <= 0) rc = -9;
            else {
                o = (uint8_t *)malloc((size_t)need);
                rc = infw_host_feed(h, win, want, last, chunk, o, need, &used, &plen, nullptr, member, at, seg_room);
                if (rc == 0 && plen != need) rc = -9;
            }
        }
        free(win);
        ++n_win;
        if (rc == 0 && (used < 0 || used > want || (last && used != want))) rc = -9;
        if (rc == 0 && total + plen > out_cap) rc = -5;
        if (rc == 0 && plen) memcpy(out + total, o, (size_t)plen);
        free(o);
        if (rc != 0) break;
        total += plen;
        if (last) break;
        if (used == 0 && plen == 0) {
            grow = want < 32 ? 64 : 2 * want;
            continue;
        }
        pos += used;
        grow = 0;
        ++i;
    }
    infw_host_close(h);
    *plain_len = total;
    if (windows) *windows = n_win;
    return rc;
}

#ifdef INFW_HOST_MAIN
static std::vector<uint8_t> slurp_file(const std::string &path) {
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
static uint64_t g_rng = 88172645463325252ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static bool check(int k, const char *what, int64_t c, bool is_good, const std::vector<uint8_t> &comp, const std::vector<uint8_t> &want,
                  const std::vector<int64_t> &sizes, int32_t chunk) {
    static std::vector<uint8_t> out((size_t)1 << 22);  // (the windows' own outputs are the exact-size blocks)
    int64_t plen = 0, at = -1, wins = 0;
    int32_t member = -1;
    const size_t room = is_good ? want.size() : out.size();
    if (out.size() < room) out.resize(room);
    const int32_t rc = infw_host_run(comp.data(), (int64_t)comp.size(), sizes.data(), (int64_t)sizes.size(), chunk, out.data(), (int64_t)room, &plen,
                                     &member, &at, &wins, 3);
    const bool ok = is_good ? rc == 0 && (size_t)plen == want.size() && (want.empty() || memcmp(out.data(), want.data(), want.size()) == 0)
                            : rc >= 1 && rc <= 11 && member >= 0 && at >= 0 && at <= (int64_t)comp.size();
    if (!ok) fprintf(stderr, "case %d %s %lld chunk %d: status %d\n", k, what, (long long)c, chunk, rc);
    return ok;
}

// <dir> <cases> [<fill> <grid>]: the files tests/test_device_gunzip_window_sanitize.py writes (case_K.gz, case_K.plain,
// case_K.info: "<1: good> <chunk>")
int main(int argc, char **argv) {
    if (argc != 3 && argc != 5) return 2;
    if (argc == 5) infs_host_set_launch(atoi(argv[3]), atoi(argv[4]));
    const std::string dir = argv[1];
    const int cases = atoi(argv[2]);
    long good = 0, bad = 0, cuts = 0, windows = 0;
    for (int k = 0; k < cases; ++k) {
        const std::string stem = dir + "/case_" + std::to_string(k);
        const std::vector<uint8_t> comp = slurp_file(stem + ".gz"), want = slurp_file(stem + ".plain"), info = slurp_file(stem + ".info");
        int flag = 0, chunk = 64;
        if (sscanf(std::string(info.begin(), info.end()).c_str(), "%d %d", &flag, &chunk) != 2) return 4;
        const bool is_good = flag & 1;
        std::vector<int64_t> sizes;  // one seeded schedule: 64 bytes to the whole file
        for (int64_t left = (int64_t)comp.size(); left > 0;) {
            const int64_t s = 64 + (int64_t)(rnd() % (uint64_t)(comp.size() > 64 ? comp.size() - 63 : 1));
            sizes.push_back(s);
            left -= s;
            ++windows;
        }
        if (!check(k, "schedule", -1, is_good, comp, want, sizes, chunk)) return 5;
        (is_good ? good : bad)++;
        if (comp.size() > 1500 || !(flag & 2)) continue;
        for (size_t c = 0; c <= comp.size(); ++c, ++cuts)  // every cut
            if (!check(k, "cut", (int64_t)c, is_good, comp, want, std::vector<int64_t>{(int64_t)c}, 64)) return 5;
    }
    printf("window inflate driver ok: %ld good, %ld bad, %ld cuts, %ld windows\n", good, bad, cuts, windows);
    return 0;
}
#endif

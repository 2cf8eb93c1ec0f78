"""The member decoder of the device inflate (csrc/bdx_inflate_core.h as plain C++) under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone driver with exact-size heap buffers runs every member of tests/inflate_cases.py
and of tests/inflate_edge_cases.py (the streams zlib's encoder never writes, good and bad), every prefix of the small ones
and some ten thousand corrupted ones.  This is where the out-of-bounds handling of bad members is
proven: a read one byte outside a member or a write one byte outside its slot is the sanitizer's to report."""
import os
import subprocess

import numpy as np

import helpers as H
import inflate_cases as IC
import inflate_edge_cases as EC
from test_sanitizers import ENV, SAN

INFLATE_DRIVER = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bdx_inflate_core.h"

static InfShared S;  // one for all members, back to back

static std::vector<uint8_t> slurp(const std::string& path) {
    std::vector<uint8_t> all;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(3); }
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + got);
    fclose(f);
    return all;
}

// exact sizes: the member ends its allocation, the slot is exactly plen bytes
static int32_t run(const uint8_t* comp, size_t clen, int32_t plen, std::vector<uint8_t>* got) {
    uint8_t* in = (uint8_t*)malloc(clen ? clen : 1);
    uint8_t* out = (uint8_t*)malloc(plen > 0 ? (size_t)plen : 1);
    if (clen) memcpy(in, comp, clen);
    int32_t st = -2;
    inf_decode_member(S, clen ? in : in + 1, (int)clen, plen > 0 ? out : out + 1, plen, &st);
    if (got) got->assign(out, out + (plen > 0 && st == 0 ? plen : 0));
    free(out);
    free(in);
    return st;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const std::string dir = argv[1];
    const int cases = atoi(argv[2]);
    INF_PHASE(inf_ph_tables(S, t))
    long good = 0, bad = 0, mangled = 0;
    uint64_t rng = 88172645463325252ull;
    for (int k = 0; k < cases; ++k) {
        const std::vector<uint8_t> comp = slurp(dir + "/member_" + std::to_string(k) + ".gz");
        const std::vector<uint8_t> want = slurp(dir + "/member_" + std::to_string(k) + ".plain");
        const std::vector<uint8_t> info = slurp(dir + "/member_" + std::to_string(k) + ".info");  // "<plen> <1: good>"
        long plen = 0;
        int is_good = 0;
        if (sscanf(std::string(info.begin(), info.end()).c_str(), "%ld %d", &plen, &is_good) != 2) return 4;
        std::vector<uint8_t> got;
        const int32_t st = run(comp.data(), comp.size(), (int32_t)plen, &got);
        if (is_good ? (st != 0 || got != want) : st <= 0) { fprintf(stderr, "member %d: status %d\n", k, st); return 5; }
        (is_good ? good : bad)++;
        if (comp.size() > 4000) continue;
        for (size_t cut = 0; cut < comp.size(); ++cut)  // every prefix is refused
            if (run(comp.data(), cut, (int32_t)plen, nullptr) <= 0) { fprintf(stderr, "member %d cut at %zu accepted\n", k, cut); return 6; }
        for (int r = 0; r < 400; ++r) {  // corrupted bytes anywhere, the header and the trailer included; slots too small and too large
            std::vector<uint8_t> c = comp;
            for (int j = 0; j < 1 + r % 3; ++j) {
                rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
                c[rng % c.size()] ^= (uint8_t)(1u << ((rng >> 32) & 7));
            }
            const long p = r % 5 == 0 ? plen / 2 : r % 7 == 0 ? plen + 100 : plen;
            (void)run(c.data(), c.size(), (int32_t)p, nullptr);
            ++mangled;
        }
    }
    printf("inflate driver ok: %ld good, %ld bad, %ld mangled\n", good, bad, mangled);
    return 0;
}
'''


def test_inflate_decoder_under_asan_ubsan(tmp_path):
    edge_bad = [m for m, _ in EC.bad_edge_members()]
    members = list(IC.good_members()) + list(IC.bad_members()) + list(EC.good_edge_members()) + edge_bad
    for k, m in enumerate(members):
        (tmp_path / ("member_%d.gz" % k)).write_bytes(m.comp)
        (tmp_path / ("member_%d.plain" % k)).write_bytes(m.plain or b"")
        (tmp_path / ("member_%d.info" % k)).write_text("%d %d\n" % (m.plen, m.plain is not None))
    src = tmp_path / "inflate_driver.cpp"
    src.write_text(INFLATE_DRIVER)
    exe = str(tmp_path / "inflate_driver")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-I", os.path.join(H.ROOT, "biodemux.jl_amd", "csrc"), "-o", exe, str(src)])
    out = subprocess.run([exe, str(tmp_path), str(len(members))], env=ENV, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "inflate driver ok: %d good, %d bad" % (len(IC.good_members()) + len(EC.good_edge_members()),
                                                   len(IC.bad_members()) + len(edge_bad)) in out.stdout
    assert int(out.stdout.split()[-2]) >= 400 * sum(len(m.comp) <= 4000 for m in members)

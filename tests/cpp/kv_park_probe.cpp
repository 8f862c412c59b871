// kv_park_probe.cpp — the blob layout of zgml_amd/csrc/kv_park.h on the CPU, as a stand-alone program (tests/test_kv_park_host.py
// compares its output with the numpy model of tests/kv_park_model.py). The header is the rule; added here is only the way through it.
//   kv_park_probe layout <n> <flags> <lanes.bin|-> <n_lanes> <cap|-> <out.bin>
//       what a park checks and writes on the host: prints "bytes <kvp_park_bytes>" and "ok <total>" or "refused: <text>"; on ok
//       out.bin holds <total> bytes — header, directory, zeroed gaps, every other payload byte 0xEE
//   kv_park_probe check <blob.bin|-> <bytes|-> <lanes.bin|-> <n_lanes>
//       what a resume checks: prints "ok <n> <n_lanes>" or "refused: <text>"
// lanes.bin: zgml_kv_lane records back to back; "-": a NULL table / a NULL blob / cap or bytes = the true size.
// Build: g++ -O2 -std=c++17 -I include.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../zgml_amd/csrc/kv_park.h"

static bool read_file(const char* path, std::vector<char>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return fprintf(stderr, "kv_park_probe: cannot read %s\n", path), false;
    char buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) out->insert(out->end(), buf, buf + got);
    fclose(f);
    return true;
}

static void say_refused(uint64_t lane, const char* why) {
    if (lane == zgml::kKvpNoLane)
        printf("refused: %s\n", why);
    else
        printf("refused: lane %llu: %s\n", (unsigned long long)lane, why);
}

// "-": NULL; else the file's records
static bool read_lanes(const char* path, std::vector<zgml_kv_lane>* lanes, const zgml_kv_lane** table) {
    *table = nullptr;
    if (!strcmp(path, "-")) return true;
    std::vector<char> raw;
    if (!read_file(path, &raw) || raw.size() % sizeof(zgml_kv_lane)) return false;
    lanes->resize(raw.size() / sizeof(zgml_kv_lane) + 1); // (+ 1: a table of no records is still not NULL)
    memcpy(lanes->data(), raw.data(), raw.size());
    *table = lanes->data();
    return true;
}

int main(int argc, char** argv) {
    std::vector<zgml_kv_lane> lanes;
    const zgml_kv_lane* table;
    uint64_t lane;
    const char* why = nullptr;
    if (argc == 8 && !strcmp(argv[1], "layout")) {
        const uint32_t n = (uint32_t)strtoul(argv[2], nullptr, 10), flags = (uint32_t)strtoul(argv[3], nullptr, 10);
        const uint64_t n_lanes = strtoull(argv[5], nullptr, 10);
        if (!read_lanes(argv[4], &lanes, &table)) return 1;
        const uint64_t bytes = zgml::kvp_park_bytes(table, n_lanes, n, flags);
        printf("bytes %llu\n", (unsigned long long)bytes);
        std::vector<char> blob(bytes ? bytes : 1, (char)0xEE);
        std::vector<zgml::KvpLaneRec> dir(n_lanes < (1u << 20) ? n_lanes : 0);
        const uint64_t cap = strcmp(argv[6], "-") ? strtoull(argv[6], nullptr, 10) : bytes;
        const uint64_t total = zgml::kvp_park_check(table, n_lanes, n, flags, blob.data(), cap, dir.data(), &lane, &why);
        if (!total) return say_refused(lane, why), 0;
        const bool empty = !n || !n_lanes;
        zgml::kvp_write_header(blob.data(), n_lanes, n, flags, total, dir.data());
        if (!empty) zgml::kvp_zero_gaps(blob.data(), dir.data(), n_lanes, n);
        printf("ok %llu\n", (unsigned long long)total);
        FILE* f = fopen(argv[7], "wb");
        if (!f || fwrite(blob.data(), 1, total, f) != total) return fprintf(stderr, "kv_park_probe: cannot write %s\n", argv[7]), 1;
        fclose(f);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "check")) {
        std::vector<char> blob;
        const bool null_blob = !strcmp(argv[2], "-");
        if (!null_blob && !read_file(argv[2], &blob)) return 1;
        const uint64_t bytes = strcmp(argv[3], "-") ? strtoull(argv[3], nullptr, 10) : blob.size();
        const uint64_t n_lanes = strtoull(argv[5], nullptr, 10);
        if (!read_lanes(argv[4], &lanes, &table)) return 1;
        blob.resize(blob.size() + 64); // (a `bytes` beyond the file reads zeros, not beyond the vector)
        zgml::KvpHeader h;
        std::vector<zgml::KvpLaneRec> dir(n_lanes < (1u << 20) ? n_lanes : 0);
        if (!zgml::kvp_check_blob(null_blob ? nullptr : blob.data(), bytes, table, n_lanes, &h, dir.data(), &lane, &why)) return say_refused(lane, why), 0;
        printf("ok %u %llu\n", h.n, (unsigned long long)h.n_lanes);
        return 0;
    }
    fprintf(stderr, "usage: kv_park_probe layout <n> <flags> <lanes.bin|-> <n_lanes> <cap|-> <out.bin>\n       kv_park_probe check <blob.bin|-> <bytes|-> <lanes.bin|-> <n_lanes>\n");
    return 2;
}

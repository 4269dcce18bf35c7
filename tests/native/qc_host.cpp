// qc_host.cpp — the inspector's kernels (elementary_amd/csrc/qc.hip) emulated lane by lane with the functions of qc.h, against the
// header's scalar twin; and the associativity of the run summaries on random flag strings. A stand-alone program (tests/test_qc_host.py
// builds and runs it):
//   qc_host assoc <seed> <rounds>
//       random strings of flags with empty, all-set and all-clear stretches, random split points: combine(summary(a), summary(b)) ==
//       summary(a || b), three-way splits in both association orders, and push-by-push == combine of one-frame leaves.
//   qc_host emulate <channels> <frames> <blockSize> <setBlocks> <silence> <clip> <clipRun> <dropout> <bucket> <pairs a:b,...|-> <in> <out>
//       `in`: float32 [channels][frames]. The programme is cut into launch sets of setBlocks blocks laid out [block][channel][blockSize]
//       (the last one cut), each run through the phases of elemhip_qc_tiles / _pairs / _fold, 128 emulated lanes per workgroup. The
//       carried states must equal the twin's byte for byte; `out` receives the reports, the pair sums and the overview.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "qc.h"

using namespace qc;

template <class U> static Runs<U> summary(const std::vector<int>& f, size_t lo, size_t hi, U minRun) {
    // a restatement by scanning: the head, the tail, the closed runs in between
    Runs<U> r = runs_empty<U>();
    r.len = (U)(hi - lo);
    size_t i = lo;
    while (i < hi && f[i]) ++i;
    r.head = (U)(i - lo);
    if (i == hi) { r.tail = r.len; return r; }
    size_t j = hi;
    while (j > lo && f[j - 1]) --j;
    r.tail = (U)(hi - j);
    while (i < j) {
        if (!f[i]) { ++i; continue; }
        size_t k = i;
        while (k < j && f[k]) ++k;
        if ((U)(k - i) >= minRun) runs_close<U>(r, (U)(k - i), (U)i);
        i = k;
    }
    return r;
}
template <class U> static bool same(const Runs<U>& a, const Runs<U>& b) { return memcmp(&a, &b, sizeof a) == 0; }

static int assoc(unsigned seed, int rounds) {
    std::mt19937 rng(seed);
    long checked = 0;
    for (int round = 0; round < rounds; ++round) {
        const size_t n = rng() % 97;
        std::vector<int> f(n);
        const int mode = rng() % 5;         // sparse, dense, all set, all clear, long stretches
        for (size_t i = 0; i < n; ++i) f[i] = mode == 2 ? 1 : mode == 3 ? 0 : mode == 4 ? (int)((i / (1 + rng() % 9)) & 1) : (int)(rng() % (mode ? 8 : 2) != 0);
        const uint32_t minRun = 1 + rng() % 5;
        size_t a = n ? rng() % (n + 1) : 0, b = n ? rng() % (n + 1) : 0;
        if (a > b) std::swap(a, b);
        const Runs<uint32_t> whole = summary<uint32_t>(f, 0, n, minRun);
        const Runs<uint32_t> s0 = summary<uint32_t>(f, 0, a, minRun), s1 = summary<uint32_t>(f, a, b, minRun), s2 = summary<uint32_t>(f, b, n, minRun);
        const Runs<uint32_t> left = runs_combine<uint32_t>(runs_combine<uint32_t>(s0, s1, (uint32_t)a, minRun), s2, (uint32_t)b, minRun);
        const Runs<uint32_t> right = runs_combine<uint32_t>(s0, runs_combine<uint32_t>(s1, s2, (uint32_t)b, minRun), (uint32_t)a, minRun);
        const Runs<uint32_t> two = runs_combine<uint32_t>(summary<uint32_t>(f, 0, b, minRun), s2, (uint32_t)b, minRun);
        Runs<uint32_t> pushed = runs_empty<uint32_t>(), leaves = runs_empty<uint32_t>();
        for (size_t i = 0; i < n; ++i) {
            runs_push<uint32_t>(pushed, f[i] != 0, (uint32_t)i, minRun);
            Runs<uint32_t> leaf = runs_empty<uint32_t>();
            leaf.len = 1; leaf.head = leaf.tail = f[i] ? 1u : 0u;
            leaves = runs_combine<uint32_t>(leaves, leaf, (uint32_t)i, minRun);
        }
        if (!same(left, whole) || !same(right, whole) || !same(two, whole) || !same(pushed, whole) || !same(leaves, whole)) {
            fprintf(stderr, "round %d: n %zu cuts %zu %zu minRun %u mode %d differ\n", round, n, a, b, minRun, mode);
            return 1;
        }
        // the 64-bit programme takes a widened 32-bit set summary behind it
        const uint64_t p0 = ((uint64_t)1 << 33) + rng() % 1000;
        Runs<uint64_t> prog = summary<uint64_t>(f, 0, a, minRun);
        for (uint64_t* at : {&prog.longestAt, &prog.firstAt}) if (*at != none<uint64_t>()) *at += p0;
        Runs<uint32_t> rest = summary<uint32_t>(f, a, n, minRun);
        for (uint32_t* at : {&rest.longestAt, &rest.firstAt}) if (*at != none<uint32_t>()) *at -= (uint32_t)a;
        Runs<uint64_t> wide = summary<uint64_t>(f, 0, n, minRun);
        for (uint64_t* at : {&wide.longestAt, &wide.firstAt}) if (*at != none<uint64_t>()) *at += p0;
        if (!same(runs_combine<uint64_t>(prog, widen(rest, p0 + a), p0 + a, minRun), wide)) { fprintf(stderr, "round %d: widened differs\n", round); return 1; }
        ++checked;
    }
    printf("assoc: %ld strings, all equal\n", checked);
    return 0;
}

// ---- the kernels' phases -----------------------------------------------------------------------------------------------------------------
struct Args {
    const float* src; ChannelState* state; PairState* pairState; const uint32_t* pairs;
    std::vector<Stretch<uint32_t>>* tileStretch; std::vector<double>* leafSums; std::vector<float>* tileEdge; std::vector<float>* out;
    uint64_t p0; uint32_t q0, count, blockSize, numChannels, numPairs, numTiles, tileCap, leafCap, outCount; Spec spec;
};
struct Range { uint64_t base, lo, hi; };
static Range tile_range(const Args& A, uint32_t t, uint32_t frames) {
    Range r; r.base = (A.p0 / frames + t) * frames; r.lo = r.base > A.p0 ? r.base : A.p0;
    const uint64_t end = A.p0 + A.count; r.hi = r.base + frames < end ? r.base + frames : end; if (r.hi < r.lo) r.hi = r.lo; return r;
}
static void stage(const Args& A, uint32_t c, const Range& r, float* rows) {
    if (r.hi <= r.lo) return;
    const uint32_t qa = A.q0 + (uint32_t)(r.lo - A.p0), qb = A.q0 + (uint32_t)(r.hi - A.p0), shift = (uint32_t)(r.lo - r.base);
    for (uint32_t tid = 0; tid < kThreads; ++tid) {
        if (A.blockSize & 3u) {
            for (uint32_t q = qa + tid; q < qb; q += kThreads) {
                const uint32_t blk = q / A.blockSize, f = q - blk * A.blockSize, j = q - qa + shift;
                rows[(j >> 6) * kRowStride + (j & 63u)] = A.src[((size_t)blk * A.numChannels + c) * A.blockSize + f];
            }
            continue;
        }
        for (uint32_t g = (qa >> 2) + tid; g * 4u < qb; g += kThreads) {
            const uint32_t q4 = g * 4u, blk = q4 / A.blockSize, f = q4 - blk * A.blockSize;
            const float* v = A.src + ((size_t)blk * A.numChannels + c) * A.blockSize + f;
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t q = q4 + k;
                if (q >= qa && q < qb) { const uint32_t j = q - qa + shift; rows[(j >> 6) * kRowStride + (j & 63u)] = v[k]; }
            }
        }
    }
}
static void tiles_workgroup(const Args& A, uint32_t t, uint32_t c) {
    std::vector<float> rows(kTileLeaves * kRowStride, -777.0f);
    std::vector<Stretch<uint32_t>> red(kTileLeaves);
    float leafMn[kTileLeaves], leafMx[kTileLeaves];
    const Range r = tile_range(A, t, kTileFrames);
    stage(A, c, r, rows.data());
    for (uint32_t l = 0; l < kThreads; ++l) {
        const uint64_t leafP = r.base + (uint64_t)l * kLeaf;
        const uint64_t a = leafP > r.lo ? leafP : r.lo, b = leafP + kLeaf < r.hi ? leafP + kLeaf : r.hi;
        Stretch<uint32_t> s = stretch_empty<uint32_t>();
        if (a < b) {
            const bool carried = leafP < A.p0;
            double sum = carried ? A.state[c].sum.partial : 0.0, sq = carried ? A.state[c].sq.partial : 0.0;
            const float* row = rows.data() + l * kRowStride;
            for (uint64_t P = a; P < b; ++P) {
                const Frame f = classify(row[(uint32_t)(P - leafP)], A.spec);
                stretch_push<uint32_t>(s, f, (uint32_t)(P - A.p0), A.spec);
                const double d = (double)f.x;
                sum += d; sq += d * d;
            }
            const uint32_t leaf = (uint32_t)(leafP / kLeaf - A.p0 / kLeaf);
            if (leaf >= A.leafCap) { fprintf(stderr, "leaf %u past the cap %u\n", leaf, A.leafCap); exit(2); }
            (*A.leafSums)[((size_t)c * 2u) * A.leafCap + leaf] = sum;
            (*A.leafSums)[((size_t)c * 2u + 1u) * A.leafCap + leaf] = sq;
        }
        red[l] = s; leafMn[l] = s.mn; leafMx[l] = s.mx;
    }
    for (uint32_t step = 1; step < kTileLeaves; step <<= 1)
        for (uint32_t l = 0; l < kThreads; ++l)
            if ((l & (2u * step - 1u)) == 0u) {
                uint64_t start = r.base + (uint64_t)(l + step) * kLeaf;
                start = start < r.lo ? r.lo : start > r.hi ? r.hi : start;
                red[l] = stretch_combine<uint32_t>(red[l], red[l + step], (uint32_t)(start - A.p0), A.spec);
            }
    if (t >= A.tileCap) { fprintf(stderr, "tile %u past the cap\n", t); exit(2); }
    (*A.tileStretch)[(size_t)c * A.tileCap + t] = red[0];
    const uint32_t B = A.spec.bucket;
    if (B == 0u || r.hi <= r.lo) return;
    const uint64_t gF = r.lo / B, gL = (r.hi - 1u) / B, g0 = A.p0 / B;
    for (uint32_t l = 0; l < kThreads; ++l)
        for (uint64_t g = gF + l; g <= gL; g += kThreads) {
            const uint64_t pa = g * B > r.lo ? g * B : r.lo, pb = (g + 1u) * B < r.hi ? (g + 1u) * B : r.hi;
            float mn = INFINITY, mx = -INFINITY;
            for (uint64_t P = pa; P < pb;) {
                const uint32_t j = (uint32_t)(P - r.base);
                if ((j & 63u) == 0u && P + kLeaf <= pb) { minmax_fold(mn, mx, leafMn[j >> 6], leafMx[j >> 6]); P += kLeaf; }
                else { const float x = classify(rows[(j >> 6) * kRowStride + (j & 63u)], A.spec).x; minmax_fold(mn, mx, x, x); P += 1u; }
            }
            if (pb - pa == B) {
                if (g - g0 >= A.outCount) { fprintf(stderr, "bucket past the count\n"); exit(2); }
                float* o = A.out->data() + ((size_t)c * A.outCount + (size_t)(g - g0)) * 2u; o[0] = mn; o[1] = mx;
            } else {
                float* e = A.tileEdge->data() + ((size_t)c * A.tileCap + t) * 4u + (g == gF ? 0u : 2u);
                e[0] = mn; e[1] = mx;
            }
        }
}
static void pairs_workgroup(const Args& A, uint32_t t, uint32_t k) {
    std::vector<float> rowsA(kPairLeaves * kRowStride, -777.0f), rowsB(kPairLeaves * kRowStride, -777.0f);
    const uint32_t ca = A.pairs[2u * k], cb = A.pairs[2u * k + 1u];
    const Range r = tile_range(A, t, kPairLeaves * kLeaf);
    if (r.hi <= r.lo) return;
    stage(A, ca, r, rowsA.data());
    stage(A, cb, r, rowsB.data());
    for (uint32_t l = 0; l < kPairLeaves; ++l) {
        const uint64_t leafP = r.base + (uint64_t)l * kLeaf;
        const uint64_t a = leafP > r.lo ? leafP : r.lo, b = leafP + kLeaf < r.hi ? leafP + kLeaf : r.hi;
        if (a >= b) continue;
        double acc = leafP < A.p0 ? A.pairState[k].partial : 0.0;
        for (uint64_t P = a; P < b; ++P) {
            const uint32_t j = (uint32_t)(P - leafP);
            acc += (double)classify(rowsA[l * kRowStride + j], A.spec).x * (double)classify(rowsB[l * kRowStride + j], A.spec).x;
        }
        (*A.leafSums)[((size_t)A.numChannels * 2u + k) * A.leafCap + (uint32_t)(leafP / kLeaf - A.p0 / kLeaf)] = acc;
    }
}
static Sums fold_row(Sums s, const double* leaves, uint32_t n, uint64_t p0, uint32_t count) {
    for (uint32_t i = 0; i < n; ++i) fold_leaf(s, leaves[i], i, p0, count);      // (every lane of the wave keeps the same sums)
    return s;
}
static void fold_workgroup(const Args& A, uint32_t row) {
    const uint32_t n = leaf_count(A.p0, A.count);
    if (row >= A.numChannels) {
        const uint32_t k = row - A.numChannels;
        A.pairState[k] = fold_row(A.pairState[k], A.leafSums->data() + ((size_t)A.numChannels * 2u + k) * A.leafCap, n, A.p0, A.count);
        return;
    }
    const uint32_t c = row;
    ChannelState* st = A.state + c;
    const Sums sum = fold_row(st->sum, A.leafSums->data() + ((size_t)c * 2u) * A.leafCap, n, A.p0, A.count);
    const Sums sq = fold_row(st->sq, A.leafSums->data() + ((size_t)c * 2u + 1u) * A.leafCap, n, A.p0, A.count);
    Stretch<uint64_t> S = st->s;
    ChannelState ov = *st;
    const uint32_t B = A.spec.bucket;
    const uint64_t g0 = B ? A.p0 / B : 0u;
    float* out = A.out->data() + (size_t)c * A.outCount * 2u;
    for (uint32_t t = 0; t < A.numTiles; ++t) {
        const Range r = tile_range(A, t, kTileFrames);
        S = stretch_combine<uint64_t>(S, widen((*A.tileStretch)[(size_t)c * A.tileCap + t], A.p0), r.lo, A.spec);
        if (B == 0u || r.hi <= r.lo) continue;
        const float* e = A.tileEdge->data() + ((size_t)c * A.tileCap + t) * 4u;
        const uint64_t gF = r.lo / B, gL = (r.hi - 1u) / B;
        if (has_lead(r.lo, r.hi, B)) {
            const uint64_t pb = (gF + 1u) * B < r.hi ? (gF + 1u) * B : r.hi;
            if (gF - g0 < A.outCount || ov.bCount + (uint32_t)(pb - r.lo) < B) bucket_merge(ov, e[0], e[1], (uint32_t)(pb - r.lo), B, gF, g0, out, 2u);
            else { fprintf(stderr, "a bucket completes past the count\n"); exit(2); }
        }
        if (has_trail(r.lo, r.hi, B)) bucket_merge(ov, e[2], e[3], (uint32_t)(r.hi - gL * B), B, gL, g0, out, 2u);
    }
    st->sum = sum; st->sq = sq; st->s = S; st->bMin = ov.bMin; st->bMax = ov.bMax; st->bCount = ov.bCount;
}

static int emulate(int argc, char** argv) {
    if (argc != 14) { fprintf(stderr, "usage: see the head of qc_host.cpp\n"); return 2; }
    const uint32_t ch = (uint32_t)atoi(argv[2]); const size_t n = (size_t)atoll(argv[3]);
    const uint32_t bs = (uint32_t)atoi(argv[4]), setBlocks = (uint32_t)atoi(argv[5]);
    Spec sp{(float)atof(argv[6]), (float)atof(argv[7]), (uint32_t)atoi(argv[8]), (uint32_t)atoi(argv[9]), (uint32_t)atoi(argv[10]), 0u};
    std::vector<uint32_t> pairs;
    if (strcmp(argv[11], "-") != 0) {
        std::string s = argv[11];
        for (size_t i = 0; i < s.size();) { size_t j = s.find(',', i); if (j == std::string::npos) j = s.size();
            unsigned a, b; if (sscanf(s.substr(i, j - i).c_str(), "%u:%u", &a, &b) != 2) return 2; pairs.push_back(a); pairs.push_back(b); i = j + 1; }
    }
    sp.numPairs = (uint32_t)(pairs.size() / 2u);
    if (!spec_ok(sp.silenceLevel, sp.clipLevel, sp.clipRun, sp.dropoutFrames, sp.bucket, sp.numPairs)) { fprintf(stderr, "spec refused\n"); return 2; }
    std::vector<float> x((size_t)ch * n);
    FILE* fi = fopen(argv[12], "rb");
    if (!fi || fread(x.data(), sizeof(float), x.size(), fi) != x.size()) { fprintf(stderr, "cannot read %s\n", argv[12]); return 2; }
    fclose(fi);
    // the twin
    std::vector<ChannelState> twin(ch, state_empty()), emu(ch, state_empty());
    std::vector<PairState> twinPairs(sp.numPairs, PairState{0.0, 0.0}), emuPairs(sp.numPairs, PairState{0.0, 0.0});
    const size_t buckets = sp.bucket ? n / sp.bucket : 0;
    std::vector<float> twinOv((size_t)ch * buckets * 2u), emuOv((size_t)ch * buckets * 2u);
    for (uint32_t c = 0; c < ch; ++c) channel_host(sp, twin[c], x.data() + (size_t)c * n, n, 0u, twinOv.data() + (size_t)c * buckets * 2u);
    for (uint32_t k = 0; k < sp.numPairs; ++k) pair_host(twinPairs[k], x.data() + (size_t)pairs[2u * k] * n, x.data() + (size_t)pairs[2u * k + 1u] * n, n, 0u, sp);
    // the kernels, set by set; the first set enters three frames late in its buffer (a window's q0)
    const size_t setFrames = (size_t)setBlocks * bs;
    const uint32_t tileCap = (uint32_t)(setFrames / kTileFrames + 2u), leafCap = (uint32_t)(setFrames / kLeaf + 2u);
    std::vector<Stretch<uint32_t>> tileStretch((size_t)ch * tileCap);
    std::vector<double> leafSums((size_t)(2u * ch + sp.numPairs) * leafCap);
    std::vector<float> tileEdge((size_t)ch * tileCap * 4u), out;
    uint64_t p0 = 0; size_t emitted = 0; bool first = true;
    while (p0 < n) {
        const uint32_t q0 = first && setFrames > 8 ? 3u : 0u;
        const uint32_t count = (uint32_t)std::min<size_t>(setFrames - q0, n - p0);
        first = false;
        std::vector<float> set((size_t)setBlocks * ch * bs, -555.0f);
        for (uint32_t c = 0; c < ch; ++c)
            for (uint32_t q = q0; q < q0 + count; ++q) set[((size_t)(q / bs) * ch + c) * bs + q % bs] = x[(size_t)c * n + p0 + (q - q0)];
        Args A{};
        A.src = set.data(); A.state = emu.data(); A.pairState = emuPairs.data(); A.pairs = pairs.data(); A.tileStretch = &tileStretch; A.leafSums = &leafSums;
        A.tileEdge = &tileEdge; A.out = &out; A.p0 = p0; A.q0 = q0; A.count = count; A.blockSize = bs; A.numChannels = ch; A.numPairs = sp.numPairs;
        A.numTiles = tile_count(p0, count); A.tileCap = tileCap; A.leafCap = leafCap; A.outCount = buckets_complete(p0, count, sp.bucket); A.spec = sp;
        out.assign((size_t)ch * A.outCount * 2u, -999.0f);
        for (uint32_t t = 0; t < A.numTiles; ++t) for (uint32_t c = 0; c < ch; ++c) tiles_workgroup(A, t, c);
        const uint32_t half = kPairLeaves * kLeaf, halves = (uint32_t)((p0 + count + half - 1u) / half - p0 / half);
        for (uint32_t t = 0; t < halves; ++t) for (uint32_t k = 0; k < sp.numPairs; ++k) pairs_workgroup(A, t, k);
        for (uint32_t row = 0; row < ch + sp.numPairs; ++row) fold_workgroup(A, row);
        for (uint32_t c = 0; c < ch; ++c)
            for (uint32_t b = 0; b < A.outCount; ++b) { emuOv[((size_t)c * buckets + emitted + b) * 2u] = out[((size_t)c * A.outCount + b) * 2u];
                                                        emuOv[((size_t)c * buckets + emitted + b) * 2u + 1u] = out[((size_t)c * A.outCount + b) * 2u + 1u]; }
        emitted += A.outCount; p0 += count;
    }
    int bad = 0;
    if (emitted != buckets) { fprintf(stderr, "%zu buckets emitted, %zu complete\n", emitted, buckets); bad = 1; }
    for (uint32_t c = 0; c < ch; ++c) if (memcmp(&twin[c], &emu[c], sizeof(ChannelState)) != 0) { fprintf(stderr, "channel %u: the carried state differs\n", c); bad = 1; }
    if (sp.numPairs && memcmp(twinPairs.data(), emuPairs.data(), sp.numPairs * sizeof(PairState)) != 0) { fprintf(stderr, "the pair sums differ\n"); bad = 1; }
    if (!twinOv.empty() && memcmp(twinOv.data(), emuOv.data(), twinOv.size() * sizeof(float)) != 0) { fprintf(stderr, "the overview differs\n"); bad = 1; }
    FILE* fo = fopen(argv[13], "wb");
    if (!fo) return 2;
    for (uint32_t c = 0; c < ch; ++c) { const ChannelReport r = report(sp, emu[c]); fwrite(&r, sizeof r, 1, fo); }
    for (uint32_t k = 0; k < sp.numPairs; ++k) { const double v = sums_value(emuPairs[k]); fwrite(&v, sizeof v, 1, fo); }
    if (!emuOv.empty()) fwrite(emuOv.data(), sizeof(float), emuOv.size(), fo);
    fclose(fo);
    printf("emulate: %u channels, %zu frames, block %u, sets of %u blocks: %s\n", ch, n, bs, setBlocks, bad ? "DIFFERS" : "the twin's bytes");
    return bad;
}

int main(int argc, char** argv) {
    if (argc >= 4 && strcmp(argv[1], "assoc") == 0) return assoc((unsigned)atoi(argv[2]), atoi(argv[3]));
    if (argc >= 2 && strcmp(argv[1], "emulate") == 0) return emulate(argc, argv);
    fprintf(stderr, "usage: qc_host assoc <seed> <rounds> | qc_host emulate ...\n");
    return 2;
}

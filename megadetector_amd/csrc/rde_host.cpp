// mdjpeg_repeat_detections: the host model of mdhip_repeat_detections (rde_kernels.cpp) and the backend='host' path of
// megadetector_amd/repeat_detections.py.  One box after the other, as the reference's loop goes; the decision about a pair of
// boxes is rde_match.h's, which the kernels compile too.  Built with -ffp-contract=off (see rde_match.h).
#include <vector>

#include "../../include/mdjpeg.h"
#include "rde_match.h"

extern "C" int mdjpeg_repeat_detections(const mdjpeg_rde_box* boxes, int64_t n, double iou_threshold, int category_agnostic,
                                        int32_t occurrence_threshold, int32_t chunk, uint8_t* is_candidate, int32_t* n_instances,
                                        int64_t* pairs, int64_t capacity, int64_t* needed) {
    if (rde_check_args(boxes, n, iou_threshold, chunk, is_candidate, n_instances, pairs, capacity, needed)) return MDJPEG_EINVAL;
    *needed = 0;
    std::vector<rde_pbox> cand;                   // the candidates opened so far, in order
    std::vector<int64_t> cand_row;                // their rows
    std::vector<int32_t> count;                   // their instances so far
    std::vector<int64_t> match_cand, match_row;   // every (candidate, instance) found, in the order of the instances
    size_t group_first = 0;                       // the first candidate of the current group
    for (int64_t i = 0; i < n; ++i) {
        const rde_pbox b = rde_prepare(boxes[i].x, boxes[i].y, boxes[i].w, boxes[i].h, boxes[i].group, boxes[i].category);
        if (i > 0 && boxes[i].group != boxes[i - 1].group) group_first = cand.size();
        bool found = false;
        for (size_t c = group_first; c < cand.size(); ++c)
            if (rde_match(b, cand[c], iou_threshold, category_agnostic)) {
                found = true;
                ++count[c];
                match_cand.push_back((int64_t)c);
                match_row.push_back(i);
            }
        is_candidate[i] = found ? 0 : 1;
        n_instances[i] = 0;
        if (!found) {
            match_cand.push_back((int64_t)cand.size());     // a candidate's first instance is itself
            match_row.push_back(i);
            cand.push_back(b);
            cand_row.push_back(i);
            count.push_back(1);
        }
    }
    // the instance lists of the suspicious candidates, one behind the other: by candidate, then by instance
    std::vector<int64_t> offset(cand.size(), -1);
    int64_t total = 0;
    for (size_t c = 0; c < cand.size(); ++c) {
        n_instances[cand_row[c]] = count[c];
        if (count[c] >= occurrence_threshold) {
            offset[c] = total;
            total += count[c];
        }
    }
    *needed = total;
    if (total > capacity) return MDJPEG_ECAPACITY;
    for (size_t m = 0; m < match_cand.size(); ++m) {
        int64_t& o = offset[match_cand[m]];
        if (o < 0) continue;
        pairs[2 * o] = match_row[m];
        pairs[2 * o + 1] = cand_row[match_cand[m]];
        ++o;
    }
    return MDJPEG_OK;
}

#ifdef MDRDE_ASAN_MAIN
// `make asan-rde`: the structural cases of tests/test_rde_cpu.py under AddressSanitizer + UBSan, as a program of its own
#include <stdio.h>

static int run(const char* name, const std::vector<mdjpeg_rde_box>& boxes, double thr, int agnostic, int occ,
               const std::vector<int>& want_cand, const std::vector<int64_t>& want_pairs) {
    const int64_t n = (int64_t)boxes.size();
    std::vector<uint8_t> is_cand(n);
    std::vector<int32_t> inst(n);
    int64_t needed = -1;
    int rc = mdjpeg_repeat_detections(boxes.data(), n, thr, agnostic, occ, 0, is_cand.data(), inst.data(), nullptr, 0, &needed);
    std::vector<int64_t> pairs(2 * (needed > 0 ? needed : 0));
    if (rc == MDJPEG_ECAPACITY)
        rc = mdjpeg_repeat_detections(boxes.data(), n, thr, agnostic, occ, 0, is_cand.data(), inst.data(), pairs.data(), needed, &needed);
    bool ok = rc == MDJPEG_OK && pairs == want_pairs;
    for (int64_t i = 0; ok && i < n; ++i) ok = is_cand[i] == want_cand[i];
    printf("%s: %s\n", name, ok ? "ok" : "WRONG");
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    std::vector<mdjpeg_rde_box> chain;      // box k matches box k + 1 and not box k + 2
    for (int k = 0; k < 9; ++k) chain.push_back({0.1 + 0.02 * k, 0.1, 0.2, 0.2, 0, 1});
    bad += run("drift chain", chain, 0.8, 0, 2, {1, 0, 1, 0, 1, 0, 1, 0, 1},
               {0, 0, 1, 0, 2, 2, 3, 2, 4, 4, 5, 4, 6, 6, 7, 6});
    bad += run("two groups", {{0.1, 0.1, 0.2, 0.2, 0, 1}, {0.1, 0.1, 0.2, 0.2, 1, 1}}, 0.9, 0, 1, {1, 1}, {0, 0, 1, 1});
    bad += run("malformed", {{0.1, 0.1, 0.0, 0.2, 0, 1}, {0.1, 0.1, -0.1, 0.2, 0, 1}, {0.1, 0.1, 0.0, 0.2, 0, 1}}, 0.0, 0, 2, {1, 1, 1}, {});
    bad += run("empty", {}, 0.9, 0, 1, {}, {});
    bad += run("one", {{0.1, 0.1, 0.2, 0.2, 0, 1}}, 0.9, 0, 1, {1}, {0, 0});
    int64_t needed = 0;
    mdjpeg_rde_box dec[2] = {{0.1, 0.1, 0.2, 0.2, 1, 1}, {0.1, 0.1, 0.2, 0.2, 0, 1}};
    uint8_t c2[2];
    int32_t i2[2];
    bad += mdjpeg_repeat_detections(dec, 2, 0.9, 0, 1, 0, c2, i2, nullptr, 0, &needed) != MDJPEG_EINVAL;
    return bad ? 1 : 0;
}
#endif

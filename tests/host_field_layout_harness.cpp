// host_field_layout_harness.cpp — the field models' slot maps (sparkfm_amd/csrc/fmhip_field_layout.h) as a stand-alone program under
// -fsanitize=address,undefined.  For every model and shape: each caller slot maps inside [0, total), no two share a device slot, every
// caller array is covered exactly once and has the size the C ABI documents, pack then unpack is the identity on the caller's arrays,
// and every device slot no caller slot maps to holds the pad value after pack.  Prints one "ok ..." line per case; exits 1 at the
// first failure.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../sparkfm_amd/csrc/fmhip_field_layout.h"

using namespace fmhip::host;

namespace {

using Sizes = std::map<std::pair<int, int>, size_t>;          // (array, layer) -> the doubles the caller passes

[[noreturn]] void die(const char *what, const char *model, long a, long b, long c) {
    fprintf(stderr, "%s: %s (%ld, %ld, %ld)\n", model, what, a, b, c);
    exit(1);
}

template <class Map>
void check(const char *model, const Map &m, const Sizes &want, const char *shape) {
    const size_t total = m.total();
    std::vector<char> taken(total, 0);
    std::map<std::pair<int, int>, std::vector<char>> seen;
    for (const auto &w : want) seen[w.first].assign(w.second, 0);
    size_t slots = 0;
    m.each([&](int a, int l, size_t i, size_t dev) {
        if (dev >= total) die("a slot maps outside [0, total)", model, a, l, (long)i);
        if (taken[dev]++) die("two caller slots share a device slot", model, a, l, (long)i);
        auto it = seen.find({a, l});
        if (it == seen.end() || i >= it->second.size()) die("a caller index outside its array", model, a, l, (long)i);
        if (it->second[i]++) die("a caller slot enumerated twice", model, a, l, (long)i);
        if (a >= Map::kLayered && l != 0) die("an array that is not one per layer comes with a layer", model, a, l, (long)i);
        ++slots;
    });
    for (const auto &s : seen)
        for (size_t i = 0; i < s.second.size(); ++i)
            if (!s.second[i]) die("a caller slot never enumerated", model, s.first.first, s.first.second, (long)i);
    // pack, unpack: the caller's values are distinct and exact in fp32, the pad is none of them
    std::map<std::pair<int, int>, std::vector<double>> in, out;
    double next = 1.0;
    for (const auto &w : want) {
        for (size_t i = 0; i < w.second; ++i) in[w.first].push_back(next++);
        out[w.first].assign(w.second, -1.0);
    }
    const float pad = -7.f;
    const std::vector<float> t = pack_slots(m, [&](int a, int l) { return in.at({a, l}).data(); }, pad);
    if (t.size() != total) die("pack's length", model, (long)t.size(), (long)total, 0);
    for (size_t dev = 0; dev < total; ++dev)
        if ((t[dev] == pad) != !taken[dev]) die("a pad slot does not hold the pad, or a mapped one does", model, (long)dev, 0, 0);
    unpack_slots(m, t.data(), [&](int a, int l) { return out.at({a, l}).data(); });
    if (in != out) die("pack then unpack is not the identity", model, 0, 0, 0);
    // an array the caller does not want is left alone
    auto skipped = out;
    for (auto &s : skipped) s.second.assign(s.second.size(), -2.0);
    unpack_slots(m, t.data(), [&](int a, int l) { return a == 0 ? nullptr : skipped.at({a, l}).data(); });
    for (const auto &s : skipped)
        if (s.first.first == 0 ? s.second != std::vector<double>(s.second.size(), -2.0) : s.second != in.at(s.first)) die("a skipped array", model, s.first.first, s.first.second, 0);
    printf("ok %s %s slots %zu total %zu\n", model, shape, slots, total);
}

}  // namespace

int main() {
    char shape[128];
    for (int F : {1, 17})
        for (int k : {1, 5}) {
            const int Kp = k == 1 ? 4 : 8, P = F * k, Pp = (F * Kp + 15) / 16 * 16;
            if (field_kp(k) != Kp || round16(F * Kp) != Pp) die("field_kp / round16", "shape", F, k, 0);
            snprintf(shape, sizeof shape, "F %d k %d", F, k);
            check("fwfm", FwfmSlots(F), Sizes{{{0, 0}, (size_t)F * F}}, shape);
            const FmfmSlots fm(F, k);
            if (fm.Pp != Pp || fm.total() != (size_t)Pp * Pp) die("FmFM's width", "fmfm", F, k, 0);
            check("fmfm", fm, Sizes{{{0, 0}, (size_t)F * F * k * k}}, shape);
            for (int L : {1, kFieldMaxLayers}) {
                const int32_t widths[kFieldMaxLayers] = {32, 16, 48};          // unequal, so a transposed or shifted layer lands elsewhere
                const DeepfmSlots deep(F, k, L, widths);
                Sizes sd;
                size_t deep_total = 0;
                for (int l = 0; l < L; ++l) {
                    sd[{0, l}] = (size_t)(l == 0 ? P : widths[l - 1]) * widths[l];
                    sd[{1, l}] = (size_t)widths[l];
                    deep_total += (size_t)(l == 0 ? Pp : widths[l - 1]) * widths[l] + widths[l];
                }
                sd[{2, 0}] = (size_t)widths[L - 1];
                if (deep.total() != deep_total + widths[L - 1]) die("DeepFM's total", "deepfm", F, k, L);
                snprintf(shape, sizeof shape, "F %d k %d L %d", F, k, L);
                check("deepfm", deep, sd, shape);

                const int r = 16;
                const DcnSlots dcn(F, k, L, r);
                Sizes sc;
                for (int l = 0; l < L; ++l) {
                    sc[{0, l}] = sc[{1, l}] = (size_t)P * r;
                    sc[{2, l}] = (size_t)P;
                }
                sc[{3, 0}] = (size_t)P;
                if (dcn.total() != (size_t)L * (2 * Pp * r + Pp) + Pp) die("DCN's total", "dcn", F, k, L);
                snprintf(shape, sizeof shape, "F %d k %d L %d rank %d", F, k, L, r);
                check("dcn", dcn, sc, shape);

                for (int heads : {1, 4}) {
                    const int A = heads * 16, d0 = 16;
                    const AutoIntSlots ai(F, k, L, A, d0);
                    Sizes sa;
                    for (int l = 0; l < L; ++l) sa[{0, l}] = (size_t)(l == 0 ? k : A) * 4 * A;
                    sa[{1, 0}] = (size_t)F * A;
                    if (ai.total() != (size_t)4 * A * d0 + (size_t)(L - 1) * 4 * A * A + (size_t)F * A) die("AutoInt's total", "autoint", F, k, L);
                    snprintf(shape, sizeof shape, "F %d k %d L %d heads %d x 16", F, k, L, heads);
                    check("autoint", ai, sa, shape);
                }
            }
        }
    return 0;
}

// fmhip_field_layout.h — where the field models keep their own parameter array on the device: one SLOT MAP per model (FwFM's r, FmFM's
// MM, and the one dense array D of DeepFM, DCN and AutoInt), pure host arithmetic with no HIP header.  A map's each(f) calls
// f(array, layer, index, device index) once per element of the caller's arrays, in the order the C ABI validates them; packing,
// unpacking, the layer pointers' check and the accumulators' validation (fmhip_field_model.h) all run that one enumeration, and
// tests/host_field_layout_harness.cpp runs it under the sanitizers.  Not installed, not part of the ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace fmhip {
namespace host {

constexpr int kFieldMaxLayers = 3;          // FMHIP_{DEEPFM,DCN,AUTOINT}_MAX_LAYERS (the units assert it)
constexpr int32_t field_kp(int32_t k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 16 ? 16 : 32)); }          // the factors' padded width
constexpr int32_t round16(int32_t x) { return (x + 15) / 16 * 16; }

// FwFM: the caller's r [F][F] as it stands
struct FwfmSlots {
    static constexpr int kLayered = 0;          // the leading arrays that come one per layer
    int32_t F = 0;
    explicit FwfmSlots(int32_t fields = 0) : F(fields) {}
    size_t total() const { return (size_t)F * F; }
    static const char *name(int) { return "r"; }
    template <class Fn> void each(Fn f) const {
        for (size_t j = 0; j < total(); ++j) f(0, 0, j, j);
    }
};

// FmFM: the caller's m[f][g][d][d'] <-> MM [Pp][Pp], row f Kp + d, column g Kp + d'
struct FmfmSlots {
    static constexpr int kLayered = 0;          // the leading arrays that come one per layer
    int32_t F = 0, k = 0, Kp = 0, Pp = 0;
    FmfmSlots() = default;
    FmfmSlots(int32_t fields, int32_t factors) : F(fields), k(factors), Kp(field_kp(factors)), Pp(round16(fields * Kp)) {}
    size_t total() const { return (size_t)Pp * Pp; }
    size_t at(int f, int g, int d, int d2) const { return (((size_t)f * F + g) * k + d) * k + d2; }           // the caller's m
    size_t dev_at(int f, int g, int d, int d2) const { return ((size_t)f * Kp + d) * Pp + (size_t)g * Kp + d2; }
    static const char *name(int) { return "m"; }
    template <class Fn> void each(Fn fn) const {
        for (int f = 0; f < F; ++f)
            for (int g = 0; g < F; ++g)
                for (int d = 0; d < k; ++d)
                    for (int d2 = 0; d2 < k; ++d2) fn(0, 0, at(f, g, d, d2), dev_at(f, g, d, d2));
    }
};

// DeepFM (fm_deepfm.h): W_l [n_{l-1}][n_l] at woff[l - 1] — W_1's caller row f k + d sits at the device's row f Kp + d —, then u, then
// the b_l.  Arrays: 0 = W, 1 = b (per layer), 2 = u
struct DeepfmSlots {
    static constexpr int kLayered = 2;          // the leading arrays that come one per layer
    int32_t F = 0, k = 0, Kp = 0, Pp = 0, L = 0;
    int32_t width[kFieldMaxLayers + 1] = {};          // width[0] = Pp on the device (F k for the caller), width[l] = n_l
    int32_t woff[kFieldMaxLayers] = {}, boff[kFieldMaxLayers] = {}, uoff = 0, n_total = 0;
    DeepfmSlots() = default;
    DeepfmSlots(int32_t fields, int32_t factors, int32_t n_layers, const int32_t *widths)
        : F(fields), k(factors), Kp(field_kp(factors)), Pp(round16(fields * Kp)), L(n_layers) {
        width[0] = Pp;
        int32_t at = 0;
        for (int l = 1; l <= L; ++l) {
            width[l] = widths[l - 1];
            woff[l - 1] = at;
            at += width[l - 1] * width[l];
        }
        uoff = at;
        at += width[L];
        for (int l = 1; l <= L; ++l) {
            boff[l - 1] = at;
            at += width[l];
        }
        n_total = at;
    }
    size_t total() const { return (size_t)n_total; }
    int rows_in(int l) const { return l == 1 ? F * k : width[l - 1]; }          // the caller's n_{l-1}
    size_t dev_row(int l, int i) const { return l == 1 ? (size_t)(i / k) * Kp + i % k : (size_t)i; }          // ... and its row on the device
    static const char *name(int a) { return a == 0 ? "W" : (a == 1 ? "b" : "u"); }
    template <class Fn> void each(Fn f) const {
        for (int l = 1; l <= L; ++l) {
            const int nl = width[l];
            for (int i = 0; i < rows_in(l); ++i)
                for (int j = 0; j < nl; ++j) f(0, l - 1, (size_t)i * nl + j, woff[l - 1] + dev_row(l, i) * nl + j);
            for (int j = 0; j < nl; ++j) f(1, l - 1, (size_t)j, (size_t)boff[l - 1] + j);
        }
        for (int j = 0; j < width[L]; ++j) f(2, 0, (size_t)j, (size_t)uoff + j);
    }
};

// DCN-V2 (fm_dcn.h): per layer V_l and U_l, both transposed (V_l [r][Pp] at voff, U_l [Pp][r] at uoff), then u at hoff, then the c_l;
// the caller's slot f k + d of a width-P vector sits at f Kp + d.  Arrays: 0 = V [P][r], 1 = U [r][P], 2 = c (per layer), 3 = u
struct DcnSlots {
    static constexpr int kLayered = 3;          // the leading arrays that come one per layer
    int32_t F = 0, k = 0, Kp = 0, Pp = 0, L = 0, r = 0;
    int32_t voff[kFieldMaxLayers] = {}, uoff[kFieldMaxLayers] = {}, coff[kFieldMaxLayers] = {}, hoff = 0, n_total = 0;
    DcnSlots() = default;
    DcnSlots(int32_t fields, int32_t factors, int32_t n_layers, int32_t rank)
        : F(fields), k(factors), Kp(field_kp(factors)), Pp(round16(fields * Kp)), L(n_layers), r(rank) {
        int32_t at = 0;
        for (int l = 0; l < L; ++l) {
            voff[l] = at;
            at += r * Pp;
            uoff[l] = at;
            at += Pp * r;
        }
        hoff = at;
        at += Pp;
        for (int l = 0; l < L; ++l) {
            coff[l] = at;
            at += Pp;
        }
        n_total = at;
    }
    size_t total() const { return (size_t)n_total; }
    int P() const { return F * k; }          // the caller's width
    size_t slot(int i) const { return (size_t)(i / k) * Kp + i % k; }
    static const char *name(int a) { return a == 0 ? "V" : (a == 1 ? "U" : (a == 2 ? "c" : "u")); }
    template <class Fn> void each(Fn f) const {
        const int p = P();
        for (int l = 0; l < L; ++l) {
            for (int j = 0; j < p * r; ++j) {
                f(0, l, (size_t)j, voff[l] + (size_t)(j % r) * Pp + slot(j / r));
                f(1, l, (size_t)j, uoff[l] + slot(j % p) * r + j / p);
            }
            for (int i = 0; i < p; ++i) f(2, l, (size_t)i, coff[l] + slot(i));
        }
        for (int i = 0; i < p; ++i) f(3, 0, (size_t)i, hoff + slot(i));
    }
};

// AutoInt (fm_autoint.h): W_l [D_l][4A] transposed at woff[l] (D_0 = k with the rows of WT_0 padded to d0, D_l = A), then u [F A] at
// hoff.  Arrays: 0 = W (per layer), 1 = u
struct AutoIntSlots {
    static constexpr int kLayered = 1;          // the leading arrays that come one per layer
    int32_t F = 0, k = 0, L = 0, A = 0, d0 = 0;
    int32_t woff[kFieldMaxLayers] = {}, hoff = 0, n_total = 0;
    AutoIntSlots() = default;
    AutoIntSlots(int32_t fields, int32_t factors, int32_t n_layers, int32_t width, int32_t first_stride)
        : F(fields), k(factors), L(n_layers), A(width), d0(first_stride) {
        int32_t at = 0;
        for (int l = 0; l < L; ++l) {
            woff[l] = at;
            at += 4 * A * stride_of(l);
        }
        hoff = at;
        n_total = at + F * A;
    }
    size_t total() const { return (size_t)n_total; }
    int rows_of(int l) const { return l == 0 ? k : A; }          // the caller's D_l
    int stride_of(int l) const { return l == 0 ? d0 : A; }       // ... and the device's
    static const char *name(int a) { return a == 0 ? "W" : "u"; }
    template <class Fn> void each(Fn f) const {
        const int N = 4 * A;
        for (int l = 0; l < L; ++l)
            for (int dd = 0; dd < rows_of(l); ++dd)
                for (int n = 0; n < N; ++n) f(0, l, (size_t)dd * N + n, woff[l] + (size_t)n * stride_of(l) + dd);
        for (int i = 0; i < F * A; ++i) f(1, 0, (size_t)i, (size_t)hoff + i);
    }
};

// CIN (fm_cin.h): W_l [H_l][hp_l][Fp] at woff[l - 1] (hp_1 = Fp = F rounded up to 16, hp_l = H_{l-1} above), field j of a row at
// position pos(j) — the MFMA order, its own inverse —, then u [H_1 + .. + H_L] at uoff.  Arrays: 0 = W [H_l][H_{l-1}][F] (per layer),
// 1 = u
struct CinSlots {
    static constexpr int kLayered = 1;          // the leading arrays that come one per layer
    int32_t F = 0, k = 0, Fp = 0, L = 0;
    int32_t H[kFieldMaxLayers + 1] = {};          // H[0] = F, H[l] = H_l
    int32_t woff[kFieldMaxLayers] = {}, uoff = 0, n_total = 0;
    CinSlots() = default;
    CinSlots(int32_t fields, int32_t factors, int32_t n_layers, const int32_t *maps) : F(fields), k(factors), Fp(round16(fields)), L(n_layers) {
        H[0] = F;
        int32_t at = 0;
        for (int l = 1; l <= L; ++l) {
            H[l] = maps[l - 1];
            woff[l - 1] = at;
            at += H[l] * stored(l) * Fp;
        }
        uoff = at;
        for (int l = 1; l <= L; ++l) at += H[l];
        n_total = at;
    }
    size_t total() const { return (size_t)n_total; }
    int stored(int l) const { return l == 1 ? Fp : H[l - 1]; }          // the device's H_{l-1}
    static int pos(int j) { return (j & ~15) + 4 * (j & 3) + ((j >> 2) & 3); }
    static const char *name(int a) { return a == 0 ? "W" : "u"; }
    template <class Fn> void each(Fn f) const {
        for (int l = 1; l <= L; ++l)
            for (int h = 0; h < H[l]; ++h)
                for (int i = 0; i < H[l - 1]; ++i)
                    for (int j = 0; j < F; ++j)
                        f(0, l - 1, ((size_t)h * H[l - 1] + i) * F + j, woff[l - 1] + ((size_t)h * stored(l) + i) * Fp + pos(j));
        for (int i = 0; i < n_total - uoff; ++i) f(1, 0, (size_t)i, (size_t)uoff + i);
    }
};

// AFM (fm_afm.h): W [t][Kp] (the caller's row of k floats at the head of the device's row of Kp: a lane of the forward reads Kp / 4
// consecutive floats of it), then b [t], h [t] and p [Kp].  Arrays: 0 = W [t][k], 1 = b, 2 = h, 3 = p
struct AfmSlots {
    static constexpr int kLayered = 0;          // the leading arrays that come one per layer
    int32_t F = 0, k = 0, Kp = 0, t = 0;
    AfmSlots() = default;
    AfmSlots(int32_t fields, int32_t factors, int32_t attention) : F(fields), k(factors), Kp(field_kp(factors)), t(attention) {}
    size_t total() const { return (size_t)t * Kp + 2 * (size_t)t + Kp; }
    static const char *name(int a) { return a == 0 ? "W" : (a == 1 ? "b" : (a == 2 ? "h" : "p")); }
    template <class Fn> void each(Fn f) const {
        for (int n = 0; n < t; ++n)
            for (int d = 0; d < k; ++d) f(0, 0, (size_t)n * k + d, (size_t)n * Kp + d);
        for (int n = 0; n < t; ++n) f(1, 0, (size_t)n, (size_t)t * Kp + n);
        for (int n = 0; n < t; ++n) f(2, 0, (size_t)n, (size_t)t * Kp + t + n);
        for (int d = 0; d < k; ++d) f(3, 0, (size_t)d, (size_t)t * Kp + 2 * (size_t)t + d);
    }
};

// PNN (fm_pnn.h): DeepFM's order — W_l at woff[l - 1], then u, then the b_l — with a taller W_1: the caller's n_0 = F k + G rows
// ([s | g], G = F (F - 1) / 2 pairs i < j, ascending in i, then in j) sit in n0p rows on the device: row f k + d at f Kp + d, the
// pair (i, j) in its Gram tile (i / 16, j / 16) at the tile's first row + (i % 16) 16 + j % 16.  The tiles on and above the diagonal
// follow one another behind the Pp field rows in ascending (mt, nt); a tile keeps its first ns slices of 16 rows — those that hold a
// pair: 16 off the diagonal, min(F - 16 mt, 16) - 1 on it.  Arrays: 0 = W, 1 = b (per layer), 2 = u
struct PnnSlots {
    static constexpr int kLayered = 2;          // the leading arrays that come one per layer
    int32_t F = 0, k = 0, Kp = 0, Pp = 0, G = 0, L = 0;
    int32_t width[kFieldMaxLayers + 1] = {};          // width[0] = n0p on the device (F k + G for the caller), width[l] = n_l
    int32_t woff[kFieldMaxLayers] = {}, boff[kFieldMaxLayers] = {}, uoff = 0, n_total = 0;
    int32_t tile_off[4][4] = {};          // [mt][nt]: the tile's first row of W_1
    PnnSlots() = default;
    PnnSlots(int32_t fields, int32_t factors, int32_t n_layers, const int32_t *widths)
        : F(fields), k(factors), Kp(field_kp(factors)), Pp(round16(fields * Kp)), G(fields * (fields - 1) / 2), L(n_layers) {
        int32_t at = Pp;
        for (int m = 0; m < (F + 15) / 16 && m < 4; ++m)
            for (int n = m; n < (F + 15) / 16 && n < 4; ++n) {
                tile_off[m][n] = at;
                at += 16 * slices(m, n);
            }
        width[0] = at;
        at = 0;
        for (int l = 1; l <= L; ++l) {
            width[l] = widths[l - 1];
            woff[l - 1] = at;
            at += width[l - 1] * width[l];
        }
        uoff = at;
        at += width[L];
        for (int l = 1; l <= L; ++l) {
            boff[l - 1] = at;
            at += width[l];
        }
        n_total = at;
    }
    size_t total() const { return (size_t)n_total; }
    int slices(int m, int n) const { return m != n ? 16 : (F - 16 * m < 16 ? F - 16 * m : 16) - 1; }
    int rows_in(int l) const { return l == 1 ? F * k + G : width[l - 1]; }          // the caller's n_{l-1}
    size_t pair_row(int i, int j) const { return (size_t)tile_off[i / 16][j / 16] + (i % 16) * 16 + j % 16; }
    static const char *name(int a) { return a == 0 ? "W" : (a == 1 ? "b" : "u"); }
    template <class Fn> void each(Fn f) const {
        for (int l = 1; l <= L; ++l) {
            const int nl = width[l];
            int pi = 0, pj = 0;          // the pair of the caller's row, walked with it
            for (int i = 0; i < rows_in(l); ++i) {
                size_t row = (size_t)i;
                if (l == 1 && i < F * k) row = (size_t)(i / k) * Kp + i % k;
                else if (l == 1) {
                    if (++pj >= F) pj = ++pi + 1;
                    row = pair_row(pi, pj);
                }
                for (int j = 0; j < nl; ++j) f(0, l - 1, (size_t)i * nl + j, woff[l - 1] + row * nl + j);
            }
            for (int j = 0; j < nl; ++j) f(1, l - 1, (size_t)j, (size_t)boff[l - 1] + j);
        }
        for (int j = 0; j < width[L]; ++j) f(2, 0, (size_t)j, (size_t)uoff + j);
    }
};

// the caller's arrays -> the device's one array; src(array, layer): the array's doubles.  The elements no slot maps to: `pad`
template <class Map, class Src>
std::vector<float> pack_slots(const Map &m, Src src, float pad) {
    std::vector<float> t(m.total(), pad);
    m.each([&](int a, int l, size_t i, size_t dev) { t[dev] = (float)src(a, l)[i]; });
    return t;
}

// ... and back; dst(array, layer): where the array goes, or NULL for one the caller does not want
template <class Map, class Dst>
void unpack_slots(const Map &m, const float *t, Dst dst) {
    m.each([&](int a, int l, size_t i, size_t dev) {
        if (double *p = dst(a, l)) p[i] = t[dev];
    });
}

}  // namespace host
}  // namespace fmhip

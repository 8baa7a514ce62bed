// Host-side probe of the quad workspace record layout (alqp_quad.hpp: QCfg). For every compiled (nx, nu) and dtype it
// dumps the workspace word of every element a quad kernel addresses, through the layout's own accessors: rec_base,
// RSTR, w, lbase / lstride / lanes_of for the L chunks (Quad::lchunk), the field offsets with the head / tail form of
// ld_slots / st_slots, and the whole-field form fw / lp / wn that ld_field / ld_rep_* read. Instantiates no kernel: built
// with hipcc on a machine without a GPU and called through ctypes by tests/test_quad_record_layout_cpu.py.
// TEST INFRASTRUCTURE: the product path never loads this.
#include "alqp_dims.hpp"
#include "alqp_quad.hpp"

namespace {

using alqp::Fld;
using alqp::QCfg;

// One element per accessed word of a record:
//   kind 0: L chunk (a = slot s, b = chunk c, lane = the storing lane), i = word inside the 4-word chunk
//   kind 1 + f: vector field f (QCfg field order oY .. oC), a = slot m of the lane, i = 0
// rel: word from the instance's record start (rec_base) at stage 0; alt: the same element through fw / lp (-1 for L);
// chunk: 1 if rel is the first word of a 4-word per-lane access (L chunks, head chunks of ld_slots / st_slots)
struct El { int kind, a, b, lane, i, rel, alt, chunk; };

template <typename real, int NX, int NU>
struct Probe {
    using C = QCfg<real, NX, NU>;

    static constexpr Fld field(int f) {
        return f == 0 ? Fld(C::oY) : f == 1 ? Fld(C::oZ) : f == 2 ? Fld(C::oR) : f == 3 ? Fld(C::oS) : f == 4 ? Fld(C::oLE)
             : f == 5 ? Fld(C::oUS) : f == 6 ? Fld(C::oQ) : f == 7 ? Fld(C::oq) : Fld(C::oC);
    }
    template <int S>
    static void vec(int f, int &n, El *out) {
        const Fld fl = field(f);
        constexpr int H = 4 * (S / 4);
        for (int q = 0; q < 4; ++q)
            for (int m = 0; m < S; ++m) {
                // ld_slots / st_slots: head chunk c at w(h + 16 c) + 4 q, tail at w(t) + 4 q + (m - H)
                const int rel = m < H ? C::w(fl.h + 16 * (m / 4)) + 4 * q + m % 4 : C::w(fl.t) + 4 * q + (m - H);
                const int alt = C::template fw<S>(fl, C::template lp<S>(m, q));
                if (out) out[n] = El{1 + f, m, 0, q, 0, rel, alt, m < H && m % 4 == 0 ? 1 : 0};
                ++n;
            }
    }
    static int elements(El *out) {
        int n = 0;
        for (int s = 0; s < C::SH; ++s)
            for (int c = 0; c <= s; ++c)
                for (int ql = 0; ql < C::lanes_of(s); ++ql)
                    for (int i = 0; i < 4; ++i) {
                        // Quad::lchunk
                        const int rel = C::w(C::oL + C::lbase(s) + c * C::lstride(s)) + 4 * ql + i;
                        if (out) out[n] = El{0, s, c, ql, i, rel, -1, i == 0 ? 1 : 0};
                        ++n;
                    }
        for (int f = 0; f < C::NF; ++f) {
            const int S = C::fslots(f);
            if (S == C::SY) vec<C::SY>(f, n, out);
            else if (S == 4) vec<4>(f, n, out);
            else vec<C::SW>(f, n, out);
        }
        return n;
    }
    // ints: RECW, RSTR, IL, SH, SW, SY, NLAST, element count, sizeof(real)
    static void meta(long *m) {
        m[0] = C::RECW; m[1] = C::RSTR; m[2] = C::IL; m[3] = C::SH; m[4] = C::SW; m[5] = C::SY; m[6] = C::NLAST;
        m[7] = elements(nullptr); m[8] = sizeof(real);
    }
    // words[b][t][e] = rec_base(b, T) + t * RSTR + rel(e)   (Quad::recp(t) of instance b)
    static long words(int B, int T, El *el, long *words) {
        const int ne = elements(el);
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < T; ++t)
                for (int e = 0; e < ne; ++e)
                    words[((long)b * T + t) * ne + e] = (long)(C::rec_base(b, T) + (size_t)t * C::RSTR) + el[e].rel;
        return (long)C::ws_words(B, T);
    }
};

template <typename real>
int dispatch(int nx, int nu, int B, int T, long *meta, El *el, long *words, long *ws_words) {
#define X(NX, NU)                                                                   \
    if (nx == NX && nu == NU) {                                                     \
        if (meta) Probe<real, NX, NU>::meta(meta);                                  \
        if (el && words) *ws_words = Probe<real, NX, NU>::words(B, T, el, words);   \
        return 0;                                                                   \
    }
    ALQP_FOR_EACH_DIMS(X)
#undef X
    return -1;
}

}  // namespace

extern "C" int quad_layout_probe(int is_f64, int nx, int nu, int B, int T, long *meta, int *el, long *words,
                                 long *ws_words) {
    static_assert(sizeof(El) == 8 * sizeof(int), "El is 8 ints");
    return is_f64 ? dispatch<double>(nx, nu, B, T, meta, reinterpret_cast<El *>(el), words, ws_words)
                  : dispatch<float>(nx, nu, B, T, meta, reinterpret_cast<El *>(el), words, ws_words);
}

#!/usr/bin/env python
"""Writes monohair_amd/csrc/mh_key_blocks.h: four taps x NI items of the search kernel's key bodies
(monohair_amd/csrc/pmvo_search.hip, which includes the header) as one hand-ordered inline-asm block per NI = 4, 3, 2, 1:
mh_key_block4<NI, KN>, which keys every tap (lists of more than one 64-tap group), and mh_key_blockm4<NI, KN, FOLD>, which
keys the block (one-group lists), and mh_key_walk<NB, KM, KN>, the walk of a list of known length (NB blocks in front of its seeded
last tap) as straight-line code: the statements of mh_key_blockm4, FOLD = false and FOLD = true in turn, each under its block's
number, the taps of the next block requested in front of it at constant offsets (see walk()).

Order inside a half (two taps of the same parity, items j = 0..NI-1): the instructions of one kind for all items, then the
next kind, so that every result is used NI - 1 or more instructions after it is produced; the second tap's products are
issued between the first tap's sum and subtraction.  Even taps g[0], g[2] fold into ke, odd taps g[1], g[3] into ko.

mh_key_blockm4: the four cs of an item as above (mul, mul, add each, the same order and bits), m = the minimum of the four
t' = fl(C - |cs|), and ONE key (m << 4) | block.  FORM "max" (the committed header): fl(C - x) is monotone non-increasing in x,
so m = fl(C - max |cs|) bit for bit -- v_max_f32 of |cs| of taps 0 and 2, v_max3_f32 with taps 1 and 3 (|.| as source
modifiers; a NaN operand is dropped, as its raw bits lost every minimum), one v_sub_f32: 13 full-rate instructions per item.
FORM "sub4" (the form before, kept for tools/ubench/key_block_forms.hip): four subtractions, the minimum on the raw bits with
one v_min_u32 and one v_min3_u32: 16 full-rate instructions.  Both: two items interleaved line by line, so that no result of a
pair is read by the next instruction (the lone third item of NI = 3 and NI = 1 cannot avoid it: the sum of a tap follows its
second product, and the tail max3, sub, lshl_or, min3 is one chain), four temporaries per item, kk the fourth where FOLD = false.
FOLD = false leaves the key in kk; FOLD = true folds kk and its own key into acc with one v_min3_u32, so that a pair of
blocks costs 7 half-rate instructions per item (2 x (max, max3, lshl_or) + min3) where the per-tap keys cost 12.

    python tools/gen_key_blocks.py > monohair_amd/csrc/mh_key_blocks.h
    python tools/gen_key_blocks.py --form sub4 --only-blockm4 --name mh_key_blockm4_sub4 > sub4.h     # beside it, for the micro-benchmark

tests/test_host.py compares the committed header with header() below.
"""


def block4(n):
    lines = []

    def half(ta, tb, acc):   # taps ta (place i0) and tb (place i1) into accumulator acc
        r = range(n)
        for j in r: lines.append(f"v_mul_f32_e32 %[a{j}], %[t{ta}x], %[x{j}]")
        for j in r: lines.append(f"v_mul_f32_e32 %[b{j}], %[t{ta}y], %[y{j}]")
        for j in r: lines.append(f"v_mul_f32_e32 %[c{j}], %[t{tb}x], %[x{j}]")
        for j in r: lines.append(f"v_add_f32_e32 %[a{j}], %[a{j}], %[b{j}]")
        for j in r: lines.append(f"v_mul_f32_e32 %[b{j}], %[t{tb}y], %[y{j}]")
        for j in r: lines.append(f"v_sub_f32_e64 %[a{j}], %[cc], |%[a{j}]|")
        for j in r: lines.append(f"v_add_f32_e32 %[c{j}], %[c{j}], %[b{j}]")
        for j in r: lines.append(f"v_lshl_or_b32 %[a{j}], %[a{j}], 5, %[i0]")
        for j in r: lines.append(f"v_sub_f32_e64 %[c{j}], %[cc], |%[c{j}]|")
        for j in r: lines.append(f"v_lshl_or_b32 %[c{j}], %[c{j}], 5, %[i1]")
        for j in r: lines.append(f"v_min3_u32 %[{acc}{j}], %[{acc}{j}], %[a{j}], %[c{j}]")

    half(0, 2, "e")
    half(1, 3, "o")
    return lines


WIDTH = 2   # items of a block-key block that are interleaved; the temporaries are those of WIDTH items
FORM = "max"   # "max": max of the four |cs|, one subtraction (the committed header); "sub4": four t', their minimum (the form before)


def blockm4(n, fold, width=WIDTH, form=FORM):
    lines = []
    for j0 in range(0, n, width):
        items = range(j0, min(n, j0 + width))

        def add(fmt):   # j the item, s its set of temporaries; FOLD = false: the key is made in kk itself (d), the fourth one
            for j in items: lines.append(fmt.format(j=j, s=j - j0, d=f"d{j - j0}" if fold else f"k{j}"))

        add("v_mul_f32_e32 %[a{s}], %[t0x], %[x{j}]")
        add("v_mul_f32_e32 %[b{s}], %[t0y], %[y{j}]")
        add("v_mul_f32_e32 %[c{s}], %[t2x], %[x{j}]")
        add("v_add_f32_e32 %[a{s}], %[a{s}], %[b{s}]")
        add("v_mul_f32_e32 %[b{s}], %[t2y], %[y{j}]")
        if form == "sub4":   # t' of every tap, the minimum on their raw bits
            add("v_sub_f32_e64 %[a{s}], %[cc], |%[a{s}]|")
            add("v_add_f32_e32 %[c{s}], %[c{s}], %[b{s}]")
            add("v_mul_f32_e32 %[{d}], %[t1x], %[x{j}]")
            add("v_sub_f32_e64 %[c{s}], %[cc], |%[c{s}]|")
            add("v_mul_f32_e32 %[b{s}], %[t1y], %[y{j}]")
            add("v_min_u32_e32 %[a{s}], %[a{s}], %[c{s}]")
            add("v_mul_f32_e32 %[c{s}], %[t3x], %[x{j}]")
            add("v_add_f32_e32 %[{d}], %[{d}], %[b{s}]")
            add("v_mul_f32_e32 %[b{s}], %[t3y], %[y{j}]")
            add("v_sub_f32_e64 %[{d}], %[cc], |%[{d}]|")
            add("v_add_f32_e32 %[c{s}], %[c{s}], %[b{s}]")
            add("v_sub_f32_e64 %[c{s}], %[cc], |%[c{s}]|")
            add("v_min3_u32 %[a{s}], %[a{s}], %[{d}], %[c{s}]")
        else:                # "max": the maximum of the four |cs| first, ONE t' = C - that
            add("v_mul_f32_e32 %[{d}], %[t1x], %[x{j}]")
            add("v_add_f32_e32 %[c{s}], %[c{s}], %[b{s}]")
            add("v_mul_f32_e32 %[b{s}], %[t1y], %[y{j}]")
            add("v_max_f32_e64 %[a{s}], |%[a{s}]|, |%[c{s}]|")
            add("v_mul_f32_e32 %[c{s}], %[t3x], %[x{j}]")
            add("v_add_f32_e32 %[{d}], %[{d}], %[b{s}]")
            add("v_mul_f32_e32 %[b{s}], %[t3y], %[y{j}]")
            add("v_add_f32_e32 %[c{s}], %[c{s}], %[b{s}]")
            add("v_max3_f32 %[a{s}], %[a{s}], |%[{d}]|, |%[c{s}]|")
            add("v_sub_f32_e32 %[a{s}], %[cc], %[a{s}]")
        if fold:
            add("v_lshl_or_b32 %[a{s}], %[a{s}], 4, %[ib]")
            add("v_min3_u32 %[m{j}], %[m{j}], %[k{j}], %[a{s}]")
        else:
            add("v_lshl_or_b32 %[k{j}], %[a{s}], 4, %[ib]")
    return lines


def emitm(n, fold, width=WIDTH, form=FORM):
    lines = blockm4(n, fold, width, form)
    w = min(n, width)
    body = "\n".join('                "%s%s"' % (l, "\\n\\t" if i < len(lines) - 1 else "") for i, l in enumerate(lines))
    if fold:
        outs = ([f'[m{j}] "+v"(acc[{j}])' for j in range(n)] + [f'[{c}{s}] "=&v"({c}[{s}])' for c in "abcd" for s in range(w)])
        kin = [f'[k{j}] "v"(kk[{j}])' for j in range(n)]
    else:
        outs = ([f'[k{j}] "=&v"(kk[{j}])' for j in range(n)] + [f'[{c}{s}] "=&v"({c}[{s}])' for c in "abc" for s in range(w)])
        kin = []
    ins = ", ".join([f'[t{u}x] "v"(g[{u}].x), [t{u}y] "v"(g[{u}].y)' for u in range(4)] +
                    [f'[x{j}] "v"(DX[{j}]), [y{j}] "v"(DY[{j}])' for j in range(n)] + kin +
                    ['[cc] "s"(MH_KEY_C)', '[ib] "s"(ib)'])
    head = "if" if fold else "else"
    cond = " constexpr (FOLD)" if fold else ""
    return (f"        {head}{cond} {{\n            asm volatile(\n{body}\n                : {', '.join(outs)}\n                : {ins}\n"
            f'                : "memory");\n        }}\n')


def emitm_n(n, width=WIDTH, form=FORM):
    head = "if" if n == 4 else "else if"
    return f"    {head} constexpr (NI == {n}) {{\n" + emitm(n, True, width, form) + emitm(n, False, width, form) + "    }\n"


HEADM = """
// the block-key body: ib = the block's number in its list (0..15)
template <int NI, int KN, bool FOLD>
__device__ __forceinline__ void mh_key_blockm4(unsigned (&acc)[KN], unsigned (&kk)[KN], const float2 (&g)[4],
                                               const float (&DX)[KN], const float (&DY)[KN], int ib) {
    static_assert(NI >= 1 && NI <= 4 && NI <= KN, "mh_key_blockm4: 1..4 items");
    constexpr int NW = NI < %d ? NI : %d;
    float a[NW], b[NW], c[NW];
    [[maybe_unused]] float d[NW];
"""


def emit(n):
    lines = block4(n)
    body = "\n".join('            "%s%s"' % (l, "\\n\\t" if i < len(lines) - 1 else "") for i, l in enumerate(lines))
    outs = ", ".join([f'[e{j}] "+v"(ke[{j}])' for j in range(n)] + [f'[o{j}] "+v"(ko[{j}])' for j in range(n)] +
                     [f'[{c}{j}] "=&v"({c}[{j}])' for c in "abc" for j in range(n)])
    ins = ", ".join([f'[t{u}x] "v"(g[{u}].x), [t{u}y] "v"(g[{u}].y)' for u in range(4)] +
                    [f'[x{j}] "v"(DX[{j}]), [y{j}] "v"(DY[{j}])' for j in range(n)] +
                    ['[cc] "s"(MH_KEY_C)', '[i0] "s"(ib)', '[i1] "s"(ib + 1)'])
    head = "if" if n == 4 else "else if"
    return (f"    {head} constexpr (NI == {n}) {{\n        asm volatile(\n{body}\n            : {outs}\n            : {ins}\n"
            f'            : "memory");\n    }}\n')


HEAD = """// generated by tools/gen_key_blocks.py -- do not edit (what the block is and why it is one asm statement: pmvo_search.hip)
template <int NI, int KN>
__device__ __forceinline__ void mh_key_block4(unsigned (&ke)[KN], unsigned (&ko)[KN], const float2 (&g)[4],
                                              const float (&DX)[KN], const float (&DY)[KN], int ib) {
    static_assert(NI >= 1 && NI <= 4 && NI <= KN, "mh_key_block4: 1..4 items");
    float a[NI], b[NI], c[NI];
"""


WALKS = (12,)   # blocks of the lists that get a walk: 49 taps (7 x 7), the last tap seeded


def walk(nb):
    """The statements of the walk of nb blocks: block i from ga (i even, FOLD = false) or gb (i odd, FOLD = true), the taps of
    block i + 1 requested in front of it from t2 at constant offsets; an odd last block folds alone."""
    out = []
    for i in range(nb):
        cur, nxt = ("ga", "gb") if i % 2 == 0 else ("gb", "ga")
        if i + 1 < nb:
            out.append(" ".join(f"{nxt}[{u}] = t2[{2 * (4 * (i + 1) + u)}];" for u in range(4)))
        out.append(f"mh_key_blockm4<KM, KN, {'true' if i % 2 else 'false'}>(acc, kk, {cur}, DX, DY, {i});")
    if nb % 2:
        out.append("for (int j = 0; j < KM; ++j) acc[j] = min(acc[j], kk[j]);")
    return out


HEADW = """
// the walk of a list of known length: the NB blocks in front of its seeded last tap as straight-line code -- the parity of a
// block, its number and the offsets of its taps from t2 (tap 0's (tx, ty); a tap record is two float2) are constants, kk is
// named only here.  ga holds block 0's taps on entry.
template <int NB, int KM, int KN>
__device__ __forceinline__ void mh_key_walk(unsigned (&acc)[KN], float2 (&ga)[4], const float2 *__restrict__ t2,
                                            const float (&DX)[KN], const float (&DY)[KN]) {
    static_assert(%s, "mh_key_walk: a generated length");
    unsigned kk[KN];
    [[maybe_unused]] float2 gb[4];
"""


def emitw(nb, first):
    body = "".join(f"        {l}\n" for l in walk(nb))
    return f"    {'if' if first else 'else if'} constexpr (NB == {nb}) {{\n{body}    }}\n"


def header(width=WIDTH, form=FORM):
    return (HEAD + "".join(emit(n) for n in (4, 3, 2, 1)) + "}\n" +
            HEADM % (width, width) + "".join(emitm_n(n, width, form) for n in (4, 3, 2, 1)) + "}\n" +
            HEADW % " || ".join(f"NB == {nb}" for nb in WALKS) + "".join(emitw(nb, i == 0) for i, nb in enumerate(WALKS)) + "}\n")


if __name__ == "__main__":
    import argparse
    # --width W: another interleave of mh_key_blockm4; --form sub4: the four-subtraction block; --name N: the function under another
    # name, so that tools/ubench/key_block_forms.hip can hold both forms (the committed header is WIDTH, FORM, mh_key_blockm4)
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=WIDTH)
    ap.add_argument("--form", choices=("max", "sub4"), default=FORM)
    ap.add_argument("--name", default="mh_key_blockm4")
    ap.add_argument("--only-blockm4", action="store_true", help="leave mh_key_block4 out (a second include beside the header)")
    args = ap.parse_args()
    text = header(args.width, args.form)
    if args.only_blockm4:
        text = text[text.index(HEADM[:40]):text.index(HEADW[:40])]
    print(text.replace("mh_key_blockm4", args.name), end="")

// png_reader.cpp -- PNG -> float RGB for image textures (trc_host_load_png), with its own inflater: libtrc_host.so links
// nothing but pthread, as trc_host_write_png writes its own deflate.
//
// The reference loads uv_test/uv_test.png and its PBR maps through MTKTextureLoader with sRGB off and the origin flipped
// vertically (AAPLRenderer.mm:349-447) and samples `.rgb`; this reader returns exactly that: byte / 255 per channel, no gamma,
// grey replicated, alpha dropped, rows bottom-up (row 0 at v = 0, the layout of trc_host_load_hdr).
//
// Formats (PNG specification, ISO/IEC 15948): bit depth 8, colour types 0 / 2 / 4 / 6, not interlaced, scanline filters
// 0-4 -- the formats of the reference's seven PNGs.  Palette, 16-bit and Adam7 files are TRC_ERR_UNSUPPORTED; a bad chunk
// CRC, a bad Adler-32, a truncated or malformed stream, or an image of more than 2^28 pixels is TRC_ERR_INVALID_ARG.
// Inflate (RFC 1951): stored, fixed and dynamic Huffman blocks, decoded canonically by code length (counts + sorted
// symbols, as in M. Adler's public-domain puff.c description of the format).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tracer_abi.h"

namespace {

struct Inflater {
    const uint8_t* in; size_t n, pos = 0;
    uint32_t bitbuf = 0; int bitcnt = 0;
    std::vector<uint8_t>& out; size_t limit;       // output stops being accepted past `limit` bytes (the expected image size)
    bool err = false;
    Inflater(const uint8_t* d, size_t len, std::vector<uint8_t>& o, size_t lim) : in(d), n(len), out(o), limit(lim) {}

    int bits(int need) {                            // `need` <= 16 bits, LSB first; sets err past the end of the input
        uint32_t v = bitbuf;
        while (bitcnt < need) {
            if (pos >= n) { err = true; return 0; }
            v |= (uint32_t)in[pos++] << bitcnt;
            bitcnt += 8;
        }
        bitbuf = v >> need; bitcnt -= need;
        return (int)(v & ((1u << need) - 1u));
    }

    struct Huff { short count[16]; short symbol[288]; };
    // canonical code from lengths; false on an over-subscribed set (an incomplete one is allowed, as zlib allows it for
    // single-code distance sets; decoding a code that does not exist is then an error)
    static bool build(Huff& h, const short* length, int n) {
        std::memset(h.count, 0, sizeof h.count);
        for (int s = 0; s < n; ++s) h.count[length[s]]++;
        if (h.count[0] == n) return true;
        int left = 1;
        for (int len = 1; len < 16; ++len) { left <<= 1; left -= h.count[len]; if (left < 0) return false; }
        short offs[16]; offs[1] = 0;
        for (int len = 1; len < 15; ++len) offs[len + 1] = offs[len] + h.count[len];
        for (int s = 0; s < n; ++s) if (length[s] != 0) h.symbol[offs[length[s]]++] = (short)s;
        return true;
    }
    int decode(const Huff& h) {
        int code = 0, first = 0, index = 0;
        for (int len = 1; len < 16; ++len) {
            code |= bits(1);
            if (err) return -1;
            const int count = h.count[len];
            if (code - count < first) return h.symbol[index + (code - first)];
            index += count; first += count; first <<= 1; code <<= 1;
        }
        err = true;                                  // ran out of codes
        return -1;
    }
    bool put(uint8_t b) { if (out.size() >= limit) { err = true; return false; } out.push_back(b); return true; }

    bool stored() {
        bitbuf = 0; bitcnt = 0;                      // to a byte boundary
        if (pos + 4 > n) return false;
        const unsigned len = in[pos] | (unsigned)in[pos + 1] << 8, nlen = in[pos + 2] | (unsigned)in[pos + 3] << 8;
        pos += 4;
        if (len != (~nlen & 0xFFFFu) || pos + len > n || out.size() + len > limit) return false;
        out.insert(out.end(), in + pos, in + pos + len);
        pos += len;
        return true;
    }
    bool codes(const Huff& lencode, const Huff& distcode) {
        static const short lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        static const short lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        static const short dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                        4097, 6145, 8193, 12289, 16385, 24577};
        static const short dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
        for (;;) {
            int sym = decode(lencode);
            if (err || sym < 0) return false;
            if (sym < 256) { if (!put((uint8_t)sym)) return false; continue; }
            if (sym == 256) return true;
            sym -= 257;
            if (sym >= 29) return false;
            const size_t len = (size_t)lbase[sym] + bits(lext[sym]);
            const int dsym = decode(distcode);
            if (err || dsym < 0 || dsym >= 30) return false;
            const size_t dist = (size_t)dbase[dsym] + bits(dext[dsym]);
            if (err || dist > out.size() || out.size() + len > limit) return false;
            const size_t from = out.size() - dist;
            for (size_t k = 0; k < len; ++k) out.push_back(out[from + k]);
        }
    }
    bool fixed() {
        static Huff lencode, distcode;
        static const bool ready = [] {
            short lengths[288];
            int s = 0;
            for (; s < 144; ++s) lengths[s] = 8;
            for (; s < 256; ++s) lengths[s] = 9;
            for (; s < 280; ++s) lengths[s] = 7;
            for (; s < 288; ++s) lengths[s] = 8;
            build(lencode, lengths, 288);
            for (s = 0; s < 30; ++s) lengths[s] = 5;
            build(distcode, lengths, 30);
            return true;
        }();
        (void)ready;
        return codes(lencode, distcode);
    }
    bool dynamic() {
        static const short order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        const int nlen = bits(5) + 257, ndist = bits(5) + 1, ncode = bits(4) + 4;
        if (err || nlen > 286 || ndist > 30) return false;
        short lengths[320];
        int idx = 0;
        for (; idx < ncode; ++idx) lengths[order[idx]] = (short)bits(3);
        for (; idx < 19; ++idx) lengths[order[idx]] = 0;
        if (err) return false;
        Huff lencode, distcode;
        if (!build(lencode, lengths, 19)) return false;
        idx = 0;
        while (idx < nlen + ndist) {
            int sym = decode(lencode);
            if (err || sym < 0) return false;
            if (sym < 16) { lengths[idx++] = (short)sym; continue; }
            short len = 0;
            int rep;
            if (sym == 16) { if (idx == 0) return false; len = lengths[idx - 1]; rep = 3 + bits(2); }
            else if (sym == 17) rep = 3 + bits(3);
            else rep = 11 + bits(7);
            if (err || idx + rep > nlen + ndist) return false;
            while (rep--) lengths[idx++] = len;
        }
        if (lengths[256] == 0) return false;         // no end-of-block code
        if (!build(lencode, lengths, nlen) || !build(distcode, lengths + nlen, ndist)) return false;
        return codes(lencode, distcode);
    }
    bool run() {
        int last;
        do {
            last = bits(1);
            const int type = bits(2);
            if (err) return false;
            bool ok = false;
            if (type == 0) ok = stored();
            else if (type == 1) ok = fixed();
            else if (type == 2) ok = dynamic();
            if (!ok || err) return false;
        } while (!last);
        return true;
    }
};

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

uint32_t crc32(const uint8_t* p, size_t n) {
    struct Table {
        uint32_t t[256];
        Table() {
            for (uint32_t i = 0; i < 256; ++i) {
                uint32_t c = i;
                for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
                t[i] = c;
            }
        }
    };
    static const Table table;
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table.t[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

uint8_t paeth(int a, int b, int c) {
    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (uint8_t)(pa <= pb && pa <= pc ? a : (pb <= pc ? b : c));
}

}  // namespace

extern "C" trc_status trc_host_load_png(const char* path, uint32_t* width, uint32_t* height, float** rgb) {
    if (!path || !width || !height || !rgb) return TRC_ERR_INVALID_ARG;
    *rgb = nullptr; *width = *height = 0;
    FILE* f = std::fopen(path, "rb");
    if (!f) return TRC_ERR_INVALID_ARG;
    std::vector<uint8_t> d;
    {
        uint8_t chunk[1 << 16];
        size_t got;
        while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) d.insert(d.end(), chunk, chunk + got);
        std::fclose(f);
    }
    static const uint8_t kSig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (d.size() < 8 || std::memcmp(d.data(), kSig, 8) != 0) return TRC_ERR_INVALID_ARG;

    // chunks: every CRC checked; IHDR first, the IDATs concatenated, IEND last
    uint32_t W = 0, H = 0, ctype = 0;
    bool have_ihdr = false, have_iend = false;
    std::vector<uint8_t> z;
    for (size_t pos = 8; !have_iend;) {
        if (pos + 12 > d.size()) return TRC_ERR_INVALID_ARG;                          // truncated
        const uint32_t len = be32(&d[pos]);
        if (len > 0x7FFFFFFFu || d.size() - pos - 12 < len) return TRC_ERR_INVALID_ARG;
        const uint8_t* type = &d[pos + 4];
        const uint8_t* data = &d[pos + 8];
        if (crc32(type, (size_t)len + 4) != be32(data + len)) return TRC_ERR_INVALID_ARG;
        pos += (size_t)len + 12;
        if (!have_ihdr) {
            if (std::memcmp(type, "IHDR", 4) != 0 || len != 13) return TRC_ERR_INVALID_ARG;
            W = be32(data); H = be32(data + 4);
            const uint8_t depth = data[8], compression = data[10], filter = data[11], interlace = data[12];
            ctype = data[9];
            if (W == 0 || H == 0 || W > 0x7FFFFFFFu || H > 0x7FFFFFFFu || compression != 0 || filter != 0 || interlace > 1)
                return TRC_ERR_INVALID_ARG;
            if ((unsigned long long)W * H > (1ull << 28)) return TRC_ERR_INVALID_ARG;
            if (depth != 8 || interlace != 0 || !(ctype == 0 || ctype == 2 || ctype == 4 || ctype == 6)) return TRC_ERR_UNSUPPORTED;
            have_ihdr = true;
        } else if (std::memcmp(type, "IDAT", 4) == 0) {
            z.insert(z.end(), data, data + len);
        } else if (std::memcmp(type, "IEND", 4) == 0) {
            have_iend = true;
        } else if (std::memcmp(type, "IHDR", 4) == 0) {
            return TRC_ERR_INVALID_ARG;
        }                                                                              // ancillary chunks (and PLTE, unused here): skipped
    }
    if (z.size() < 6) return TRC_ERR_INVALID_ARG;

    // zlib wrapper (RFC 1950): deflate, window <= 32 K, no preset dictionary, header check, Adler-32 of the output at the end
    const uint8_t cmf = z[0], flg = z[1];
    if ((cmf & 0x0F) != 8 || (cmf >> 4) > 7 || (flg & 0x20) || ((unsigned)cmf << 8 | flg) % 31u != 0) return TRC_ERR_INVALID_ARG;
    const uint32_t channels = ctype == 0 ? 1u : (ctype == 2 ? 3u : (ctype == 4 ? 2u : 4u));
    const size_t stride = (size_t)W * channels;
    const size_t expect = (stride + 1) * H;
    std::vector<uint8_t> raw;
    Inflater inf(z.data() + 2, z.size() - 2, raw, expect);
    if (!inf.run() || raw.size() != expect) return TRC_ERR_INVALID_ARG;
    if (inf.pos + 4 > inf.n) return TRC_ERR_INVALID_ARG;                               // the Adler-32 follows at a byte boundary
    {
        uint32_t a = 1, b = 0;
        for (size_t i = 0; i < raw.size();) {
            const size_t end = std::min(raw.size(), i + 5552);                         // no overflow before the modulo
            for (; i < end; ++i) { a += raw[i]; b += a; }
            a %= 65521u; b %= 65521u;
        }
        if (((b << 16) | a) != be32(inf.in + inf.pos)) return TRC_ERR_INVALID_ARG;
    }

    // unfilter in place (each scanline: filter byte + stride bytes; bpp = channels at bit depth 8)
    const size_t bpp = channels;
    for (uint32_t y = 0; y < H; ++y) {
        uint8_t* row = &raw[(size_t)y * (stride + 1)];
        const uint8_t ft = row[0];
        uint8_t* cur = row + 1;
        const uint8_t* up = y ? cur - (stride + 1) : nullptr;
        if (ft > 4) return TRC_ERR_INVALID_ARG;
        for (size_t i = 0; i < stride; ++i) {
            const int a = i >= bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
            int v = cur[i];
            if (ft == 1) v += a;
            else if (ft == 2) v += b;
            else if (ft == 3) v += (a + b) >> 1;
            else if (ft == 4) v += paeth(a, b, c);
            cur[i] = (uint8_t)v;
        }
    }

    float* out = (float*)std::malloc((size_t)W * H * 3 * sizeof(float));
    if (!out) return TRC_ERR_OOM;
    for (uint32_t y = 0; y < H; ++y) {
        const uint8_t* src = &raw[(size_t)y * (stride + 1) + 1];
        float* dst = out + (size_t)(H - 1 - y) * W * 3;                                // bottom-up
        for (uint32_t x = 0; x < W; ++x) {
            const uint8_t* p = src + (size_t)x * channels;
            const bool grey = channels <= 2;
            dst[3 * x]     = (float)p[0] / 255.0f;
            dst[3 * x + 1] = (float)p[grey ? 0 : 1] / 255.0f;
            dst[3 * x + 2] = (float)p[grey ? 0 : 2] / 255.0f;
        }
    }
    *width = W; *height = H; *rgb = out;
    return TRC_OK;
}

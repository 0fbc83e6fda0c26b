// host_bases.h - what the host code of the stages reads and writes besides coordinates: a volume's bases as byte codes, decoded from the 2-bit words the
// device holds, and alignment columns as codes, four to a byte.  The only host definitions of either in the library; the copies of the words from the
// device are fetch_words / fetch_read_words in necat_hip.hip.  No HIP in this header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace necat_host {

// A volume's 2-bit words on the host, or a slice of them: w[0] is word `word0` of the volume (base g in bits 2 (g & 31) of word g >> 5), seq_off the
// volume's sequence offsets.  decode reads words (seq_off[id] + from) >> 5 .. (seq_off[id] + to - 1) >> 5 only, forward strand positions.
struct BaseWords {
    const uint64_t* w = nullptr;
    uint64_t word0 = 0;
    const uint64_t* seq_off = nullptr;

    uint64_t size(int64_t id) const { return seq_off[id + 1] - seq_off[id]; }
    uint8_t base(uint64_t g) const { return (uint8_t)((w[(g >> 5) - word0] >> ((g & 31) * 2)) & 3); }
    // a slice as the kernels address one (nw::Seq, dal::DSeq): base i is base g0 + dir * i of the volume, complemented when comp; one code 0 .. 3 per byte
    void slice(int64_t g0, int dir, int comp, int64_t len, uint8_t* dst) const
    {
        for (int64_t i = 0; i < len; ++i) { const uint8_t c = base((uint64_t)(g0 + (int64_t)dir * i)); dst[i] = comp ? (uint8_t)(3 - c) : c; }
    }
    // the n bases that start at base g of the volume, or their reverse complement
    void stretch(uint64_t g, int64_t n, int rev, uint8_t* dst) const { if (rev) slice((int64_t)g + n - 1, -1, 1, n, dst); else slice((int64_t)g, 1, 0, n, dst); }
    // bases [from, to) of sequence `id`, or of its reverse complement (coordinates on that strand)
    void decode(int64_t id, int rev, int64_t from, int64_t to, uint8_t* dst) const
    {
        if (rev) slice((int64_t)seq_off[id + 1] - 1 - from, -1, 1, to - from, dst); else slice((int64_t)seq_off[id] + from, 1, 0, to - from, dst);
    }
    // the whole sequence on one strand
    void strand(int64_t id, int rev, std::vector<uint8_t>& dst) const { dst.resize(size(id)); decode(id, rev, 0, (int64_t)dst.size(), dst.data()); }
};

// the n bases from base `from` on of NECAT pac bytes - what a volume file holds, first base of a byte in its top two bits - one code 0 .. 3 per byte
inline void decode_pac(const uint8_t* pac, uint64_t from, uint64_t n, uint8_t* dst)
{
    for (uint64_t i = 0; i < n; ++i) { const uint64_t g = from + i; dst[i] = (uint8_t)((pac[g >> 2] >> ((~g & 3) << 1)) & 3); }
}

// the code of one alignment column from its two gapped characters (necat_onc_align_batch's codes: 0 match, 1 query base only, 2 template base only, 3 mismatch)
inline uint8_t col_code(char q, char t) { return q == '-' ? 2 : (t == '-' ? 1 : (q == t ? 0 : 3)); }

// n columns four to a byte, column j in bits 2 (j & 3) of byte j >> 2; writes (n + 3) / 4 bytes.  code(j): column j's code.
template <class Code>
inline void pack_cols_of(size_t n, uint8_t* dst, Code&& code)
{
    for (size_t j = 0; j < n; ++j) {
        if (!(j & 3)) dst[j >> 2] = 0;
        dst[j >> 2] |= (uint8_t)((code(j) & 3) << (2 * (j & 3)));
    }
}
inline void pack_cols(const uint8_t* codes, size_t n, uint8_t* dst) { pack_cols_of(n, dst, [codes](size_t j) { return codes[j]; }); }

}  // namespace necat_host

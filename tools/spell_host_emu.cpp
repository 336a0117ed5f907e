// Host emulation of phasm_amd/csrc/spell.hip.h for tests/test_spell_host_emulation.py: the kernels compiled as plain C++, threads
// one after another, so a machine without a GPU checks their indexing and logic -- the search for a chunk's piece, the walk over
// short and empty pieces, the words a fetch loads, the letters, the upper-casing in the word, the bound of the patch -- against
// the goldens, under the host sanitizers.  The reads are packed as append_packed of c_api.hip packs them (every read on a
// 16-byte boundary, one zero guard word behind it, exception records for bytes other than ACGT in a 2-bit store, 8 bits per
// base when a read has more than len / 64 + 16 of them), into buffers of exactly that size: a load or a store outside them is
// a sanitizer report.  The launches follow run_spell.
//   argv[1]: a text file
//           bits n_reads n_pieces n_seqs first_byte n_out given     (bits 0: as the library decides; first_byte a multiple of
//                                                                    16; n_out 0: the whole output; given 1: offsets follow)
//           one line per read: its bytes in hex, "-" for an empty read
//           n_pieces lines "read take"; n_seqs + 1 numbers seq_off; if given: n_pieces + 1 piece offsets
//   stdout: "bits n_bytes n_patched", the seq_byte_off, then bytes [first_byte, first_byte + n_out) of the output in hex
#include "host_emu.h"
#include <cinttypes>
#include <string>
#include "../phasm_amd/csrc/spell.hip.h"
using namespace po;

static int code_of(unsigned char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    uint32_t bits, n_reads, n_pieces, n_seqs, given;
    uint64_t first_byte, n_out;
    if (fscanf(f, "%u %u %u %u %" SCNu64 " %" SCNu64 " %u", &bits, &n_reads, &n_pieces, &n_seqs, &first_byte, &n_out, &given) != 7) return 1;
    if ((bits != 0 && bits != 2 && bits != 8) || (first_byte & 15)) return 1;
    std::vector<std::string> reads(n_reads);
    std::vector<char> line(1 << 20);
    for (uint32_t r = 0; r < n_reads; ++r) {
        if (fscanf(f, "%1048575s", line.data()) != 1) return 1;
        const size_t n = strlen(line.data());
        if (n == 1 && line[0] == '-') continue;
        if (n & 1) return 1;
        for (size_t i = 0; i < n; i += 2) {
            unsigned v;
            if (sscanf(line.data() + i, "%2x", &v) != 1) return 1;
            reads[r].push_back((char)v);
        }
    }
    std::vector<uint32_t> piece_read(n_pieces + 1, 0), piece_take(n_pieces + 1, 0);
    for (uint32_t p = 0; p < n_pieces; ++p) {
        if (fscanf(f, "%u %u", &piece_read[p], &piece_take[p]) != 2) return 1;
        if (piece_read[p] >= n_reads || piece_take[p] > reads[piece_read[p]].size()) return 1;   // (the library refuses it on the host)
    }
    std::vector<uint64_t> seq_off(n_seqs + 1);
    for (uint32_t s = 0; s <= n_seqs; ++s)
        if (fscanf(f, "%" SCNu64, &seq_off[s]) != 1 || seq_off[s] > n_pieces || (s && seq_off[s] < seq_off[s - 1])) return 1;
    if (seq_off[0] != 0 || seq_off[n_seqs] != n_pieces) return 1;
    std::vector<uint64_t> piece_off((size_t)n_pieces + 1, 0xDEADDEADDEADull), seq_byte_off((size_t)n_seqs + 1, 0xDEADull);
    if (given)
        for (uint32_t p = 0; p <= n_pieces; ++p)
            if (fscanf(f, "%" SCNu64, &piece_off[p]) != 1) return 1;
    fclose(f);
    // ---- append_packed ----
    if (!bits) {
        bits = 2;
        for (const std::string& s : reads) {
            size_t cnt = 0;
            for (unsigned char c : s) cnt += code_of(c) < 0;
            if (cnt > s.size() / 64 + 16) bits = 8;
        }
    }
    const size_t per = 64 / bits;
    std::vector<uint64_t> words, woff;
    std::vector<uint32_t> exc_off{0}, exc_pos;
    std::vector<uint8_t> exc_byte;
    for (const std::string& s : reads) {
        const size_t off = (words.size() + 1) & ~size_t(1), nw = (s.size() + per - 1) / per;
        words.resize(off + nw + 1, 0);
        for (size_t i = 0; i < s.size(); ++i) {
            const unsigned char c = (unsigned char)s[i];
            if (bits == 8) {
                words[off + (i >> 3)] |= (uint64_t)c << ((i & 7) * 8);
            } else if (code_of(c) >= 0) {
                words[off + (i >> 5)] |= (uint64_t)code_of(c) << ((i & 31) * 2);
            } else {
                exc_pos.push_back((uint32_t)i);
                exc_byte.push_back(c);
            }
        }
        if (bits == 2) exc_off.push_back((uint32_t)exc_pos.size());
        woff.push_back(off);
    }
    // ---- run_spell ----
    uint64_t n_bytes = 0, n_patched = 0;
    std::vector<uint32_t> scan((size_t)n_pieces + 1, 0xDEADu);
    for (uint32_t p = 0; p < n_pieces; ++p) {   // the library's prefix_sum: exclusive offsets and the closing sentinel
        scan[p] = (uint32_t)n_bytes;
        n_bytes += piece_take[p];
        if (bits == 2)
            for (uint32_t e = exc_off[piece_read[p]]; e < exc_off[piece_read[p] + 1]; ++e) n_patched += exc_pos[e] < piece_take[p];
    }
    if (n_bytes > 0xFFFFFFFFull - 15) return 1;
    scan[n_pieces] = (uint32_t)n_bytes;
    if (given) {
        n_bytes = piece_off[n_pieces];   // (the offsets came with the case: an output longer than one call may make)
        for (uint32_t s = 0; s <= n_seqs; ++s) seq_byte_off[s] = piece_off[seq_off[s]];
    } else {
        LAUNCH(2, 3, k_spell_offsets(n_pieces ? scan.data() : nullptr, n_pieces, seq_off.data(), n_seqs, piece_off.data(), seq_byte_off.data()));
    }
    if (!n_out) n_out = n_bytes > first_byte ? n_bytes - first_byte : 0;
    const uint64_t n_chunks = (n_out + 15) / 16;
    std::vector<SpellChunk> out(n_chunks, SpellChunk{0xEEEEEEEEEEEEEEEEull, 0xEEEEEEEEEEEEEEEEull});
    if (n_chunks) {
        LAUNCH(3, 2, k_spell_decode(words.data(), woff.data(), bits, piece_read.data(), piece_take.data(), piece_off.data(), n_pieces, first_byte,
                                    n_chunks, out.data()));
        if (bits == 2 && !exc_pos.empty())
            LAUNCH(3, 2, k_spell_patch(piece_read.data(), piece_take.data(), piece_off.data(), n_pieces, exc_off.data(), exc_pos.data(),
                                       exc_byte.data(), first_byte, n_chunks * 16, reinterpret_cast<uint8_t*>(out.data())));
    }
    printf("%u %" PRIu64 " %" PRIu64 "\n", bits, n_bytes, n_patched);
    for (uint32_t s = 0; s <= n_seqs; ++s) printf("%" PRIu64 " ", seq_byte_off[s]);
    printf("\n");
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(out.data());
    for (uint64_t i = 0; i < n_out; ++i) printf("%02x", bytes[i]);
    printf("\n");
    return 0;
}

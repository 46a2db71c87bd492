/*
 * kgx_fq_body.h -- how the fq handler cuts a request's blocks into parts when
 * the device frames them (option "fq_body_device", kguts_fq.cpp, DESIGN.md
 * §8.14): kgx_fq_parts.h's arithmetic, used block by block.  No HIP and no
 * project header but that one: tests/native/fq_body_check.cpp compiles this
 * file alone and runs it against a byte-wise model.
 *
 * A request arrives in blocks, and every record complete within a block is
 * looked up in that block (one FamilyMapper per block), so unlike
 * kgx_f2p_process a block's last part runs whether it is full or not; only
 * the text behind the last complete record is carried into the next block.
 *
 *     begin_block(bytes the block brings, the part size)
 *     while the block has bytes left:
 *         if (beyond_limit(left)) -> the rest of the block through the host parser
 *         k = take(left); append k bytes; took(k)
 *         parse buffer[0, have) -> consumed        -- the block's last part when left == 0
 *         parsed(consumed, bytes still left in the block)
 *         move buffer[consumed, consumed + have) to the front
 *
 * A gzip body's parts end at member boundaries: take_members() instead of
 * take(), the part's bytes being the sum of its members' sizes.
 */
#pragma once

#include <algorithm>
#include <cstdint>

#include "kgx_fq_parts.h"

namespace kgx {

struct FqBodyParts {
    FqParts parts;
    uint64_t limit = 0; /* the most text one parse takes (KGX_FQ_PARSE_MAX) */

    void reset(uint64_t part_bytes, uint64_t most)
    {
        parts.reset(part_bytes);
        limit = most;
    }
    uint64_t have() const { return parts.have; }
    /* a block of n bytes begins behind the carried text.  The first part is
     * an eighth of the others when the block makes more than one (nothing
     * overlaps its parse); the room always leaves space behind the carry */
    void begin_block(uint64_t n, uint64_t part_bytes)
    {
        parts.part_bytes = std::max<uint64_t>(part_bytes, 1);
        parts.room = n / parts.part_bytes > 1 ? std::max<uint64_t>(parts.part_bytes / 8, 1) : parts.part_bytes;
        while (parts.room <= parts.have)
            parts.room *= 2;
    }
    /* a part never holds more than one parse takes, however its room has grown */
    uint64_t room() const { return std::min(parts.room, limit); }
    /* the carried text fills the limit and holds no complete record: the
     * record in progress needs a part beyond it, and the rest of the block
     * (`left` bytes) goes through the host parser */
    bool beyond_limit(uint64_t left) const { return left && parts.have >= limit; }
    uint64_t take(uint64_t left) const { return parts.have < room() ? std::min(left, room() - parts.have) : 0; }
    void took(uint64_t k) { parts.took(k); }
    /* a gzip body: the members the next part takes of those with out_len[0, n)
     * bytes of text -- as many as fit in the room behind the carry, and at
     * least one; *bytes = their text */
    uint32_t take_members(const uint32_t *out_len, uint32_t n, uint64_t *bytes) const
    {
        uint64_t b = 0;
        uint32_t k = 0;
        while (k < n && (k == 0 || parts.have + b + out_len[k] <= room()))
            b += out_len[k++];
        *bytes = b;
        return k;
    }
    /* not even the next member fits behind the carried text */
    bool members_beyond_limit(uint64_t bytes) const { return parts.have + bytes > limit; }
    /* after the parse of buffer[0, have): buffer[consumed, have) is carried;
     * `left`: bytes of the block still to come (0: the block's last part, and
     * the next block sets its own room) */
    void parsed(uint64_t consumed, uint64_t left) { parts.parsed(consumed, 0, left != 0); }
    /* the host parser took the part: this much text follows its last complete record */
    void carried(uint64_t bytes) { parts.have = bytes; }
    /* the request is over, or forgotten after an error */
    void forget() { parts.reset(parts.part_bytes); }
};

}  // namespace kgx

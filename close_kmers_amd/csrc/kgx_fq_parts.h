/*
 * kgx_fq_parts.h -- the part and tail arithmetic of kgx_f2p_process when a
 * part's text is framed on the device (option "fq_parse_device", kgx_fq_parse):
 * how much new text a part takes, when it runs, what is carried in front of
 * the next bytes, the line count across parts, and how a part grows when it
 * holds no complete record.  No HIP and no other project header:
 * tests/native/fq_parts_check.cpp compiles this file alone and runs it against
 * a byte-wise model.
 *
 * The part buffer holds `have` bytes: the tail carried over, then new bytes.
 *
 *     while input remains, or the input has ended and have > 0:
 *         k = take(input left); append k bytes; took(k)
 *         if (!ready(no more input in this file)) break   -- wait for the next block
 *         parse buffer[0, have) -> consumed, newlines      -- FINISHED on the file's last part
 *         parsed(consumed, newlines, more input to come)
 *         move buffer[consumed, consumed + have) to the front
 */
#pragma once

#include <algorithm>
#include <cstdint>

namespace kgx {

struct FqParts {
    uint64_t part_bytes = 0; /* a part's size as asked for (>= 1) */
    uint64_t room = 0;       /* the current part's: part_bytes, doubled while a part holds no complete record */
    uint64_t have = 0;       /* bytes in the part buffer */
    uint64_t lines = 0;      /* '\n' consumed by the parts before this one */

    void reset(uint64_t bytes)
    {
        part_bytes = room = std::max<uint64_t>(bytes, 1);
        have = lines = 0;
    }
    /* new bytes the part takes of `avail` */
    uint64_t take(uint64_t avail) const { return std::min(avail, room - have); }
    void took(uint64_t k) { have += k; }
    /* the part runs when it is full, or holds what is left of a file that has ended */
    bool ready(bool input_ended) const { return have >= room || (input_ended && have > 0); }
    /* after the parse of buffer[0, have): buffer[consumed, have) is carried.
     * A part without a complete record, with more input to come, is not run
     * again unchanged: its room doubles, so the next run holds more text (a
     * record longer than part_bytes).  Once a record is consumed the room
     * returns to part_bytes, or to the first doubling that leaves space
     * behind the carried tail. */
    void parsed(uint64_t consumed, uint64_t newlines, bool more_to_come)
    {
        lines += newlines;
        have -= consumed;
        if (!more_to_come)
            return;
        room = consumed ? part_bytes : room * 2;
        while (room <= have)
            room *= 2;
    }
    /* the file's line of an error the parse of this part reports:
     * error_newlines = '\n' in buffer[0, error_pos] */
    uint64_t error_line(uint64_t error_newlines) const { return 1 + lines + error_newlines; }
};

}  // namespace kgx

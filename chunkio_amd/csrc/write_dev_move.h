// write_dev_move.h -- the arithmetic of the batched in-place move
// (write_dev_gpu.hip: move_save, move_shift): the content of many images at
// once, each shifted onto itself by its own delta (cio_file_write_metadata's
// memmove, src/cio_file.c:1075-1145).  No HIP type, so that the same text
// compiles for the device and, stand-alone on the host, under ASan + UBSan
// (tools/move_check.cpp, `make movecheck`).  Not installed.
//
// Record i: mlen[i] bytes at base + msrc[i] move to base + msrc[i] + mdelta[i],
// |mdelta| <= 65535; a record with mlen == 0 does not move.  The planner's image
// of the SOURCE regions gives the balance, as for the append copy
// (write_dev_copy.h): S steps in all, segment k of G takes steps [k S / G,
// (k + 1) S / G), and a record's units [j0, j1) inside a segment are one
// PIECE.  A segment is a workgroup.  The units tile the destination exactly as
// copy_units tiles it, so a piece is a contiguous destination range [plo, phi)
// whose source is [plo - delta, phi - delta).
//
// The hazard.  Images are distinct and a record moves inside its image, so a
// piece's source can only be overwritten by pieces of the SAME record.  With
// delta > 0 those are the pieces below it (their destinations end at plo), and
// what they can reach of its source is [plo - delta, plo): the first
// min(delta, len) source bytes.  The rest of its source, [plo, phi - delta),
// lies in its own destination range, which only its own segment writes.  With
// delta < 0 it is mirrored: the pieces above reach the last min(-delta, len)
// source bytes.  A piece that starts its record (delta > 0) or ends it
// (delta < 0) has no such neighbour.
//
// So there are two kernels and no workgroup ever waits on another:
//   save   every segment copies that exposed part of its pieces' sources to its
//          own arena slots; nothing writes an image in this kernel.
//   shift  every segment moves the rest of each piece tile by tile, downwards
//          for delta > 0 and upwards for delta < 0, and then stores the exposed
//          part from the arena.  A tile is one wave's 4 KiB; the workgroup runs
//          one tile per wave at a time: every lane loads, the workgroup meets
//          at a barrier, every lane stores.  No tile's stores reach a source
//          the segment has yet to read, and the tiles of one such phase can
//          belong to different pieces, so a segment of a hundred 4 KiB images
//          keeps as many bytes in flight as one inside a 4 MiB image.
// Only a segment's first piece can continue a record from below and only its
// last piece can continue into the segment above, and the two can be pieces of
// different records with opposite signs, so a segment owns two slots of
// kMoveSlot bytes: slot 0 for delta > 0, slot 1 for delta < 0.
#ifndef CIOA_WRITE_DEV_MOVE_H
#define CIOA_WRITE_DEV_MOVE_H

#include <stdint.h>

#include "write_dev_copy.h"

namespace cioa {

constexpr uint32_t kMoveThreads = 512;               // one workgroup per segment
constexpr uint32_t kMoveWaves = kMoveThreads / kWave;   // 8: the tiles of one phase, one per wave
constexpr uint32_t kMoveRows = 4;                    // 16-byte units per lane per tile
constexpr uint32_t kMoveUnits = kWave * kMoveRows;   // 256 units: 4 KiB of body per tile
constexpr uint64_t kMoveSlot = 65536;                // >= the largest |delta|, a multiple of 16
constexpr uint64_t kMoveSegBytes = 2 * kMoveSlot;    // arena bytes per segment

// What one lane holds of a tile between its loads and its stores.
struct MoveRegs {
    u32x4 v[kMoveRows];
    uint8_t h, t;
};

// One tile, one WAVE: len bytes to d from s -- a head of up to 15 bytes to d's
// first 16-byte boundary, up to kMoveUnits 16-byte units, a tail of up to 15
// bytes.  Head and tail go bytewise (only a range's first and last tile have
// them); the body is read with unaligned 16-byte loads and stored with aligned
// ones, four 1 KiB rows per wave.
CIOA_COPY_FN void tile_load(MoveRegs &r, const uint8_t *d, const uint8_t *s, uint64_t len, uint32_t lane)
{
    const uint64_t dh = umin((16u - ((uint64_t) (uintptr_t) d & 15u)) & 15u, len);
    const uint64_t be = dh + ((len - dh) & ~(uint64_t) 15);
    if (lane < dh) {
        r.h = s[lane];
    }
#ifdef __HIPCC__
#pragma unroll
#endif
    for (uint32_t k = 0; k < kMoveRows; ++k) {
        const uint64_t x = dh + ((uint64_t) lane + (uint64_t) k * kWave) * kGran;
        if (x < be) {
            r.v[k] = reinterpret_cast<const Unaligned16 *>(s + x)->v;
        }
    }
    if (be + lane < len) {
        r.t = s[be + lane];
    }
}

CIOA_COPY_FN void tile_store(const MoveRegs &r, uint8_t *d, uint64_t len, uint32_t lane)
{
    const uint64_t dh = umin((16u - ((uint64_t) (uintptr_t) d & 15u)) & 15u, len);
    const uint64_t be = dh + ((len - dh) & ~(uint64_t) 15);
    if (lane < dh) {
        d[lane] = r.h;
    }
#ifdef __HIPCC__
#pragma unroll
#endif
    for (uint32_t k = 0; k < kMoveRows; ++k) {
        const uint64_t x = dh + ((uint64_t) lane + (uint64_t) k * kWave) * kGran;
        if (x < be) {
            *reinterpret_cast<u32x4 *>(d + x) = r.v[k];
        }
    }
    if (be + lane < len) {
        d[be + lane] = r.t;
    }
}

// len bytes to d from s, which may overlap it (s = d - delta), as a sequence
// of tiles: the range's head and its first kMoveUnits units, then kMoveUnits
// units each, the last tile with the range's tail -- so a range of 4 KiB at any
// alignment is ONE tile.  The sequence runs from the top when down (delta > 0)
// and from the bottom otherwise: then no tile's stores reach the source of a
// LATER tile of the sequence.  ex.tile(d, s, len) hands a tile to the
// workgroup, which runs kMoveWaves of them at a time as one PHASE: all loads,
// a barrier, all stores (a tile's stores may reach its own source, and that
// of the tiles before it, whose loads are done by then).
template <class Ex>
CIOA_COPY_FN void move_range(uint8_t *d, const uint8_t *s, uint64_t len, bool down, Ex &ex)
{
    if (len == 0) {
        return;
    }
    const uint64_t dh = umin((16u - ((uint64_t) (uintptr_t) d & 15u)) & 15u, len);
    const uint64_t nunits = (len - dh) / kGran;
    const uint64_t nt = umax(1, (nunits + kMoveUnits - 1) / kMoveUnits);
    for (uint64_t i = 0; i < nt; ++i) {
        const uint64_t k = down ? nt - 1 - i : i;
        const uint64_t lo = k == 0 ? 0 : dh + k * kMoveUnits * kGran;
        const uint64_t hi = k == nt - 1 ? len : dh + (k + 1) * kMoveUnits * kGran;
        ex.tile(d + lo, s + lo, hi - lo);
    }
}

struct MovePiece {
    uint8_t *d;            // destination of the piece's first byte
    const uint8_t *s;      // its source: d - delta
    uint64_t len;
    uint64_t sv;           // bytes other segments may overwrite: the first sv (down) or the last sv
    bool down;             // delta > 0
};

// Units [j0, j1) of a record of len bytes whose content moves to D: the
// destination range as copy_units cuts it.  false: the piece is empty.
CIOA_COPY_FN bool move_piece(MovePiece &p, uint8_t *D, int64_t delta, uint64_t len, uint64_t j0, uint64_t j1,
                             uint32_t nunits)
{
    const uint64_t dh = (uint64_t) (uintptr_t) D & 15u;
    const uint64_t end = dh + len;            // positions are relative to D - dh
    const uint64_t lo = j0 == 0 ? dh : j0 * (uint64_t) kStep;
    const uint64_t hi = j1 == nunits ? end : umin(j1 * (uint64_t) kStep, end);
    if (lo >= hi) {
        return false;
    }
    p.d = D + (lo - dh);
    p.s = p.d - delta;
    p.len = hi - lo;
    p.down = delta > 0;
    const uint64_t mag = (uint64_t) (delta > 0 ? delta : -delta);
    const bool exposed = delta > 0 ? j0 != 0 : j1 != nunits;
    p.sv = exposed ? umin(mag, p.len) : 0;
    return true;
}

// What the walk needs of one record.  A segment of small records walks a
// hundred of them; read one after the other from global memory, each costs a
// round trip that nothing hides, so the workgroup stages kMoveWindow of them at
// a time (one thread each) and walks the staged window.
struct MoveRec {
    uint64_t g;            // first step
    uint64_t src, len;     // msrc, mlen
    int64_t delta;
    uint32_t ns, pad;      // steps
};
constexpr uint32_t kMoveWindow = 256;

CIOA_COPY_FN MoveRec move_rec(const ChunkDesc *desc, const uint64_t *msrc, const uint64_t *mlen,
                              const int64_t *mdelta, uint32_t c)
{
    MoveRec r;
    r.g = desc[c].g;
    r.ns = desc[c].nsteps;
    r.src = msrc[c];
    r.len = mlen[c];
    r.delta = mdelta[c];
    r.pad = 0;
    return r;
}

// A segment's steps [t, t1), t inside record c (or in the gap before it),
// walked over the window win[] = records [c0, c0 + nw): until the steps or the
// window run out; t and c are left where the walk goes on.  slots: the
// segment's own kMoveSegBytes of the arena.  SAVE: the first kernel (exposed
// parts to the slots); otherwise the second (the shift, then the exposed parts
// back).  The caller ends the last phase (ex.end()) after the last window.
template <bool SAVE, class Ex>
CIOA_COPY_FN void move_window(uint8_t *base, uint8_t *slots, const MoveRec *win, uint32_t c0, uint32_t nw,
                              uint64_t &t, uint64_t t1, uint32_t &c, Ex &ex)
{
    while (t < t1 && c < c0 + nw) {
        const MoveRec r = win[c - c0];
        if (r.ns != 0) {
            const uint64_t j1 = umin(t1, r.g + r.ns) - r.g;
            MovePiece p;
            if (move_piece(p, base + r.src + r.delta, r.delta, r.len, t - r.g, j1, r.ns)) {
                uint8_t *slot = slots + (p.down ? 0 : kMoveSlot);
                const uint64_t keep = p.len - p.sv;          // bytes only this segment touches
                if (SAVE) {
                    move_range(slot, p.down ? p.s : p.s + keep, p.sv, false, ex);
                } else if (p.down) {
                    move_range(p.d + p.sv, p.s + p.sv, keep, true, ex);
                    move_range(p.d, slot, p.sv, false, ex);
                } else {
                    move_range(p.d, p.s, keep, false, ex);
                    move_range(p.d + keep, slot, p.sv, false, ex);
                }
            }
            t = r.g + j1;
        }
        ++c;
    }
}

// Records of 1..3 bytes have no step: one thread each, loads before stores.
CIOA_COPY_FN void move_tiny(uint8_t *base, const uint64_t *msrc, const uint64_t *mlen, const int64_t *mdelta,
                            uint32_t n, uint64_t first, uint64_t stride)
{
    for (uint64_t i = first; i < n; i += stride) {
        const uint64_t len = mlen[i];
        if (len != 0 && len < 4) {
            const uint8_t *s = base + msrc[i];
            uint8_t *d = base + msrc[i] + mdelta[i];
            const uint8_t b0 = s[0], b1 = len > 1 ? s[1] : 0, b2 = len > 2 ? s[2] : 0;
            d[0] = b0;
            if (len > 1) {
                d[1] = b1;
            }
            if (len > 2) {
                d[2] = b2;
            }
        }
    }
}

}  // namespace cioa

#endif

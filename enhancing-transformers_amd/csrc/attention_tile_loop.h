// attention_tile_loop.h — what differs between the two compilations of a kernel text (attention_kernels.h, x3_attention.h).
//   ATT_SEL(tail, aligned)   one of two token sequences
//   ATT_TILES_BEGIN / _END   the key-tile loop of a forward / dQ kernel, around ONE tile body:
//     ATT_TAIL 0: `for (int kt = 0; kt < nt; ++kt) { ... }` — the aligned kernels' loop, token for token;
//     ATT_TAIL 1: the same loop over the nt FULL tiles with `LAST` false, and behind it one more instance of the body with LAST true for the ragged tile nt.
//   ATT_UNLESS_LAST { ... }  the close of a tile (ring advance, wait for the next tile, barrier): nothing follows the ragged tile
// (Tried and dropped: a third instance for tile nt - 1, so that the loop needs no `is the ragged tile next` branch around its request.  The forward then
//  fits 130 registers instead of 194, but the compiler reloads a kernel argument inside its loop — a scalar load on the counter the fragment reads are
//  counted on — and lays dQ's three instances inside one back edge.)
#pragma once
#if ATT_TAIL
#define ATT_SEL(tail, aligned) tail
#define ATT_UNLESS_LAST if constexpr (!LAST)
#define ATT_TILES_BEGIN(kt, nt) auto att_tile = [&](const int kt, auto att_last) __attribute__((always_inline)) { [[maybe_unused]] constexpr bool LAST = decltype(att_last)::value;
#define ATT_TILES_END(kt, nt) }; for (int kt = 0; kt < nt; ++kt) att_tile(kt, std::false_type{}); att_tile(nt, std::true_type{});
#else
#define ATT_SEL(tail, aligned) aligned
#define ATT_UNLESS_LAST
#define ATT_TILES_BEGIN(kt, nt) for (int kt = 0; kt < nt; ++kt) {
#define ATT_TILES_END(kt, nt) }
#endif

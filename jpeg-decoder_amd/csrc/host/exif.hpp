// exif.hpp — the orientation tag out of the EXIF bytes the front-end keeps (Frontend::exif(): the payload behind "Exif\0\0").
// The TIFF header ("II" or "MM", magic 42, IFD0's offset), IFD0's 12-byte entries, tag 0x0112 of type SHORT and count 1: a value of
// 1..8 is the orientation.  Everything else — no EXIF, a truncated or out-of-bounds IFD, another type or count, another value — is 1,
// never an error.  Every read is checked against the blob.  (XMP orientation is not read: include/jpgpu.h.)
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace jpgpu {
namespace host {

inline uint32_t exif_orientation(const uint8_t *b, size_t len) {
    if (!b || len < 8) return 1u;
    const bool le = b[0] == 'I' && b[1] == 'I';
    if (!le && !(b[0] == 'M' && b[1] == 'M')) return 1u;
    const auto u16 = [&](size_t at) { return le ? (uint32_t)b[at] | ((uint32_t)b[at + 1] << 8) : ((uint32_t)b[at] << 8) | (uint32_t)b[at + 1]; };
    const auto u32 = [&](size_t at) { return le ? u16(at) | (u16(at + 2) << 16) : (u16(at) << 16) | u16(at + 2); };
    if (u16(2) != 42u) return 1u;
    const size_t ifd = u32(4);
    if (ifd + 2u > len) return 1u;
    const uint32_t n = u16(ifd);
    for (uint32_t k = 0; k < n; k++) {
        const size_t at = ifd + 2u + 12u * (size_t)k;
        if (at + 12u > len) return 1u;  // (an entry cut short)
        if (u16(at) != 0x0112u) continue;
        if (u16(at + 2) != 3u || u32(at + 4) != 1u) return 1u;
        const uint32_t v = u16(at + 8);
        return (v >= 1u && v <= 8u) ? v : 1u;
    }
    return 1u;
}

}  // namespace host
}  // namespace jpgpu

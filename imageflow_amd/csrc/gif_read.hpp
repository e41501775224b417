// gif_read.hpp -- what the host learns from a GIF file before the device sees it (csrc/gif_read.cpp): the logical screen,
// the colour tables as BGRA entries, and for every frame up to the one a job wants its descriptor, what its graphic control
// extension said, and its data sub-blocks gathered into one LZW stream.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ifhip {

struct GifFrameInfo {
    uint32_t left = 0, top = 0, w = 0, h = 0;
    uint32_t interlace = 0;
    uint32_t dispose = 1;                // gif::DisposalMethod: 0 Any, 1 Keep, 2 Background, 3 Previous (a frame without an extension: Keep)
    uint32_t transparent = 0xFFFFFFFFu;  // the transparent index, or none
    uint32_t delay = 0, user_input = 0;
    uint32_t min_code = 0;
    uint32_t pal_off = 0, pal_n = 0;     // the frame's palette in GifParsed::palettes: the local table, else the global one
    size_t stream_off = 0;               // in GifParsed::streams: a multiple of 16, zeros up to the next multiple and 16 bytes beyond
    uint32_t stream_len = 0;
};
struct GifParsed {
    uint32_t w = 0, h = 0;               // the logical screen
    uint32_t bg = 0;                     // Screen::new's background as a BGRA dword: the global table's entry, alpha 255; else 0
    uint32_t bg_index = 0;
    bool has_global = false;
    uint32_t global_n = 0;
    std::vector<uint32_t> palettes;      // BGRA dwords, alpha 255: the global table first, then every local one
    std::vector<uint8_t> streams;
    std::vector<GifFrameInfo> frames;    // frames 0 .. target, fewer where the file ends first
    uint32_t status = 0;                 // the IFHIP_GIF_DEC_* word of the walk; non-zero: nothing runs for the file
    int32_t repeat = -1;                 // the loop count of a NETSCAPE2.0 block in front of the walk's end (0: for ever), -1: none seen
};
// The header alone (signature, screen descriptor).  IFHIP_OK, or IFHIP_INVALID_ARGUMENT with an "ImageMalformed: GIF
// decoding error ..." message.
int parse_gif_header(const uint8_t* d, size_t len, GifParsed* out);
// The walk up to frame `target`.  Fails like parse_gif_header; everything behind the header is the status word.
int parse_gif(const uint8_t* d, size_t len, uint32_t target, GifParsed* out);
// The walk to the file's end: every frame, status 0 where the walk met nothing wrong and saw a frame at the least.
int parse_gif_all(const uint8_t* d, size_t len, GifParsed* out);
// The device part of a decode (csrc/gif_decode.hip).  files[i] == nullptr: the file's header did not parse.
int gif_decode_parsed_device(const GifParsed* const* files, uint32_t n_files, uint8_t* const* d_frames, const size_t* frame_bytes,
                             const uint32_t* strides, uint32_t* d_status, void* hip_stream);
// As gif_decode_parsed_device for ONE file, every screen: screen k (the logical screen behind frame k's blit) lies at
// d_screens + k * screen_pitch.  The file's status word goes to d_status[0]; a damaged frame anywhere: no screen is written.
int gif_decode_all_parsed_device(const GifParsed& file, uint8_t* d_screens, size_t screen_pitch, uint32_t stride, uint32_t* d_status, void* hip_stream);
const char* gif_status_text(uint32_t status);

}  // namespace ifhip

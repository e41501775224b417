// encode_handoff.hpp -- the host code that the file coders (png_encode.hip, png_quantize.hip, webp_encode.hip, gif_encode.hip)
// share around their kernels: the opening checks of ifhip_*_batch_device and the frame of the synchronous host-buffer drop-in
// ifhip_*.  A new writer brings its stage (creation and its checks included), its own argument checks and its kernels.
#pragma once
#include "hip_entry.hpp"

namespace ifhip {

// The opening of ifhip_*_batch_device for a stage with width, height and max_images: *go says whether there is a batch to
// code behind it; with IFHIP_OK and no *go the batch is empty and the entry point returns IFHIP_OK at once.
template <typename Stage>
int open_encode_batch(const Stage* stage, const uint8_t* d_images, size_t image_bytes, uint32_t stride, uint32_t n_images, const uint8_t* d_files,
                      const uint32_t* d_lengths, bool* go) {
    *go = false;
    if (!stage) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null stage");
    if (n_images == 0) return IFHIP_OK;
    if (n_images > stage->max_images) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: %u images exceed the stage capacity %u", n_images, stage->max_images);
    if (int rc = check_frames(d_images, image_bytes, stage->width, stage->height, stride, "image")) return rc;
    if (!d_files || !d_lengths) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null pointer");
    *go = true;
    return IFHIP_OK;
}

// ifhip_* on the null stream: create(&stage) makes a stage for one image, the bitmap goes up with room behind it for a file of
// the stage's bound (rounded up to 16), its length and its status word, batch(stage, frame, pitch, d_len) makes the one batch
// call (d_len + 1: the status word), and the file comes down into `out` (null: the length alone).  *word is the status word.
template <typename Stage, typename Create, typename Batch>
int encode_host_frame(const uint8_t* bgra, uint32_t w, uint32_t h, uint32_t stride, uint8_t* out, size_t capacity, size_t* len, uint32_t* word, Create create,
                      void (*destroy)(Stage*), size_t (*max_file_bytes)(const Stage*), Batch batch) {
    if (!len) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null length out-pointer");
    *len = 0;
    *word = 0;
    Stage* stage = nullptr;
    if (int rc = create(&stage)) return rc;
    struct Guard {                       // (behind the frame's block: the stage goes once the null stream has run dry)
        Stage* s;
        void (*destroy)(Stage*);
        ~Guard() { (void)hipStreamSynchronize(nullptr); destroy(s); }
    } guard{stage, destroy};
    const size_t pitch = (max_file_bytes(stage) + 15u) & ~static_cast<size_t>(15u);
    HostFrame f;
    if (int rc = f.up(bgra, w, h, stride, pitch + 16u)) return rc;
    if (int rc = batch(stage, f, pitch, reinterpret_cast<uint32_t*>(f.side_output() + pitch))) return rc;
    return f.down_file(pitch, out, capacity, len, word);
}

// what the drop-in answers for a status word that no caller can act on, or for no file at all
inline int refuse_unfitted_file(uint32_t status, size_t len) {
    if (status || !len) return fail(IFHIP_INVALID_STATE, "InvalidState: the file did not fit its worst-case size (status %u)", status);
    return IFHIP_OK;
}

}  // namespace ifhip

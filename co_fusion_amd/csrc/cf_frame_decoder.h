// cf_frame_decoder.h -- the decoder object shared by frame_decode.hip (.klg frames) and image_decode.hip (image-sequence frames).
#pragma once

#include "cf_device.h"
#include "cf_host.h"

namespace cf {

constexpr int kDecHeaderBytes = 512;   // the header's place at the front of a slot's staging block (coefficients follow, 16 B aligned)
constexpr int kMaxDecSlots = 16;

struct ImageExt;   // image_decode.hip: what cf_frame_decoder_enable_images adds
void image_ext_destroy(ImageExt* e);
void image_ext_clear_mask(ImageExt* e, int slot);   // (e may be null)


}  // namespace cf

struct cf_frame_decoder {
    cf_ctx* ctx = nullptr;
    int max_w = 0, max_h = 0, slots = 0;
    uint64_t cap_blocks = 0;
    size_t off_depth = 0, off_rgb = 0, slot_bytes = 0;   // staging block: header | coefficients | depth | rgb (host and device alike)
    hipStream_t stream = nullptr;
    hipEvent_t consumed = nullptr;
    hipEvent_t done[cf::kMaxDecSlots]{};
    uint8_t* h_slot[cf::kMaxDecSlots]{};   // pinned
    uint8_t* d_slot[cf::kMaxDecSlots]{};
    uint8_t* d_planes = nullptr;    // one set: the decoder's stream runs the frames one after the other
    float* d_depth[cf::kMaxDecSlots]{};
    uint8_t* d_rgba[cf::kMaxDecSlots]{};
    bool submitted[cf::kMaxDecSlots]{};
    // diagnostics (cf_frame_decoder_timing)
    bool timing = false;
    hipEvent_t tev[cf::kMaxDecSlots][3]{};
    bool timed[cf::kMaxDecSlots]{};
    double idct_ms = 0, finish_ms = 0;
    uint64_t frames = 0;
    cf::ImageExt* img = nullptr;    // null until cf_frame_decoder_enable_images
};

namespace cf {

// frame_decode.hip: the copies and launches of a frame whose colour lies in the slot's .klg staging (JPEG header + coefficients, or
// rgb bytes).  with_depth: the whole of cf_frame_decoder_submit's work (u16 mm depth too, timing events); without it the colour half
// alone, for an image frame whose depth comes from elsewhere.  swap: store R, G, B reversed.  The caller has ordered the stream and
// checked the frame's size.
int frame_decoder_colour(cf_frame_decoder* d, int slot, int width, int height, int color_kind, bool swap, bool with_depth);
// frame_decode.hip: reads the events of the frame timed in this slot, .klg or image, into the sums (cf_frame_decoder_timing is on)
int frame_decoder_harvest(cf_frame_decoder* d, int slot);
// image_decode.hip: reads the events of an image frame timed in this slot, if there is one, into the image sums
int image_ext_harvest(cf_frame_decoder* d, int slot);

}  // namespace cf

// hip_interop_webp_lossy_enc.rs -- the declarations of include/imageflow_hip_webp_lossy_enc.h (the device lossy WebP coder,
// csrc/vp8_encode.hip), beside the generated hip_interop.rs: that file names exactly what include/imageflow_hip.h declares,
// and this header stays apart from it until the stream-order table of the main header gains its row.
// For codecs/webp.rs: WebPEncoder::write_frame with EncoderPreset::WebPLossy (WebPEncodeBGRA / WebPEncodeBGR).
#![allow(non_camel_case_types)]
use std::os::raw::{c_int, c_void};

#[repr(C)] pub struct ifhip_webp_lossy_enc_stage { _private: [u8; 0] }
pub const IFHIP_VP8_ENC_FILE_OVERFLOW: u32 = 1;
pub const IFHIP_VP8_ENC_INTRA4: u32 = 1;       // stage flag: a macroblock may take sixteen 4x4 luma modes (B_PRED)

#[link(name = "imageflow_hip")]
extern "C" {
    pub fn ifhip_webp_lossy_enc_stage_create(stage: *mut *mut ifhip_webp_lossy_enc_stage, width: u32, height: u32, alpha_meaningful: c_int, max_images: u32) -> c_int;
    pub fn ifhip_webp_lossy_enc_stage_create_flags(stage: *mut *mut ifhip_webp_lossy_enc_stage, width: u32, height: u32, alpha_meaningful: c_int, max_images: u32, flags: u32) -> c_int;
    pub fn ifhip_webp_lossy_encode_flags(bgra: *const u8, width: u32, height: u32, stride: u32, alpha_meaningful: c_int, quality: f32, flags: u32, out: *mut u8, capacity: usize, len: *mut usize) -> c_int;
    pub fn ifhip_webp_lossy_enc_stage_destroy(stage: *mut ifhip_webp_lossy_enc_stage);
    pub fn ifhip_webp_lossy_enc_stage_max_file_bytes(stage: *const ifhip_webp_lossy_enc_stage) -> usize;
    pub fn ifhip_webp_lossy_encode_batch_device(stage: *mut ifhip_webp_lossy_enc_stage, d_images: *const u8, image_bytes: usize, stride: u32, n_images: u32, quality: f32, d_files: *mut u8, file_pitch: usize, d_lengths: *mut u32, d_status: *mut u32, hip_stream: *mut c_void) -> c_int;
    pub fn ifhip_webp_lossy_encode(bgra: *const u8, width: u32, height: u32, stride: u32, alpha_meaningful: c_int, quality: f32, out: *mut u8, capacity: usize, len: *mut usize) -> c_int;
}

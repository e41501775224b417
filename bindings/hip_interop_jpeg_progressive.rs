// hip_interop_jpeg_progressive.rs -- the declarations of include/imageflow_hip_jpeg_progressive.h (the device entropy decoder of
// progressive JPEG files, csrc/jpeg_progressive_decode.hip), beside the generated hip_interop.rs: that file names exactly what
// include/imageflow_hip.h declares, and this header stays apart from it until the stream-order table of the main header gains
// its row.  For codecs/mozjpeg_decoder.rs: MzDec::read_frame's jpeg_read_coefficients on a progressive file, and the two shim
// calls of include/imageflow_abi_subset.h that switch the jobs' decodes over.
#![allow(non_camel_case_types)]
use std::os::raw::{c_int, c_void};

#[repr(C)] pub struct ifhip_jpeg_progressive_prepared { _private: [u8; 0] }
#[repr(C)] pub struct imageflow_context { _private: [u8; 0] }
pub const IFHIP_JPEG_PROG_NO_SUCH_CODE: u32 = 1;
pub const IFHIP_JPEG_PROG_PAST_SE: u32 = 2;
pub const IFHIP_JPEG_PROG_REFINE_SIZE: u32 = 4;
pub const IFHIP_JPEG_PROG_OUT_OF_BITS: u32 = 8;
pub const IFHIP_JPEG_PROG_BOUNDS: u32 = 16;

#[link(name = "imageflow_hip")]
extern "C" {
    pub fn ifhip_jpeg_progressive_prepare(prepared: *mut *mut ifhip_jpeg_progressive_prepared, jpeg: *const u8, len: usize) -> c_int;
    pub fn ifhip_jpeg_progressive_prepared_info(prepared: *const ifhip_jpeg_progressive_prepared, width: *mut u32, height: *mut u32, n_components: *mut c_int, h_samp3: *mut u8, v_samp3: *mut u8, blocks_w3: *mut u32, blocks_h3: *mut u32, qt3x64: *mut u16, n_scans: *mut u32, n_streams: *mut u32, n_levels: *mut u32) -> c_int;
    pub fn ifhip_jpeg_progressive_prepared_destroy(prepared: *mut ifhip_jpeg_progressive_prepared);
    pub fn ifhip_jpeg_progressive_decode_batch_device(prepared: *const *const ifhip_jpeg_progressive_prepared, n_files: u32, d_coef0: *const *mut i16, d_coef1: *const *mut i16, d_coef2: *const *mut i16, plane_bytes: *const usize, d_status: *mut u32, hip_stream: *mut c_void) -> c_int;
    pub fn ifhip_jpeg_progressive_decode(jpeg: *const u8, len: usize, coef0: *mut i16, coef1: *mut i16, coef2: *mut i16, qt3x64: *mut u16, status: *mut u32) -> c_int;
    pub fn ifhip_shim_context_set_device_progressive_decoder(context: *mut imageflow_context, on: c_int) -> bool;
    pub fn ifhip_shim_device_progressive_decodes(context: *mut imageflow_context, fell_back: *mut i64) -> i64;
}

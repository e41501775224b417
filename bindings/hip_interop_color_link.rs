// hip_interop_color_link.rs -- the declarations of include/imageflow_hip_color_link.h (GRAY and LUT-based ICC profiles converted to
// sRGB through a colour link, csrc/color_link.cpp + csrc/color_link.hip), beside the generated hip_interop.rs: that file names
// exactly what include/imageflow_hip.h declares, and this header stays apart from it until the stream-order table of the main
// header gains its row.  For codecs/lcms2_transform.rs: SourceProfile::IccProfileGray and an IccProfile that carries A2B0, and
// the two shim calls of include/imageflow_abi_subset.h that switch the jobs' conversions on.
#![allow(non_camel_case_types)]
use std::os::raw::{c_int, c_void};

#[repr(C)] pub struct ifhip_color_link { _private: [u8; 0] }
#[repr(C)] pub struct imageflow_context { _private: [u8; 0] }
pub const IFHIP_COLOR_LINK_GRAY: c_int = 1;
pub const IFHIP_COLOR_LINK_RGB: c_int = 2;
pub const IFHIP_COLOR_LINK_GRID: u32 = 33;
pub const IFHIP_COLOR_KIND_GRAY: u32 = 1;
pub const IFHIP_COLOR_KIND_LUT: u32 = 2;

#[link(name = "imageflow_hip")]
extern "C" {
    pub fn ifhip_color_link_from_icc(icc: *const u8, len: usize, frame_is_gray: c_int, link: *mut *mut ifhip_color_link) -> c_int;
    pub fn ifhip_color_link_free(link: *mut ifhip_color_link);
    pub fn ifhip_color_link_kind(link: *const ifhip_color_link) -> c_int;
    pub fn ifhip_color_link_copy_nodes(link: *const ifhip_color_link, out: *mut c_void, capacity: usize, written: *mut usize) -> c_int;
    pub fn ifhip_color_link_transform(bgra: *mut u8, w: u32, h: u32, stride: u32, link: *mut ifhip_color_link) -> c_int;
    pub fn ifhip_color_link_transform_batch_device(d_bgra: *mut u8, image_bytes: usize, n_images: u32, w: u32, h: u32, stride: u32, link: *mut ifhip_color_link, hip_stream: *mut c_void) -> c_int;
    pub fn ifhip_shim_context_set_color_profile_kinds(context: *mut imageflow_context, flags: u32) -> bool;
    pub fn ifhip_shim_color_links_built(context: *mut imageflow_context) -> i64;
}

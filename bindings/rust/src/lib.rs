//! `aprilgrid::detector::TagDetector` over libaprilgrid_amd.so (MI355X / gfx950).
//!
//! The surface is the reference's (aprilgrid 0.8.0): `TagDetector::new(&TagFamily, Option<DetectorParams>)`
//! (src/detector.rs:364-406), `detect(&self, &DynamicImage) -> HashMap<u32, [(f32, f32); 4]>` (:505-540),
//! `refined_saddle_points(&self, &DynamicImage) -> Vec<Saddle>` (:408-446), `detect_kornia` behind the `kornia`
//! feature (:478-503), plus `detect_many` (no counterpart there: `detect` over a batch of equally sized frames, the
//! form that keeps a GPU busy).  The types `TagFamily`, `DetectorParams` and `Saddle` repeat the reference's
//! definitions (src/tag_families.rs:5-28, src/detector.rs:25-41, src/saddle.rs:3-15) so that a caller switches by
//! changing a `use` line; inside the reference crate the same file works as `src/amd.rs` with these three replaced by
//! `crate::` paths.
//!
//! Failure model: the reference returns no errors -- an internal failure is a panic (src/detector.rs:500), "nothing
//! found" an empty collection.  Every C entry point returns a status and never unwinds into Rust; a non-zero status
//! becomes the panic the reference's own failures are.
//!
//! Not compiled in the repository's build image (no Rust toolchain there).  The declarations of `ffi` are checked
//! against the header by the repository's CPU test-suite (tests/test_rust_binding.py).
pub mod ffi;

use std::collections::HashMap;
use std::os::raw::{c_int, c_void};
use std::sync::Mutex;

/// The reference's `GrayImagef32` (src/image_util.rs): an f32 luma plane.
pub type GrayImagef32 = image::ImageBuffer<image::Luma<f32>, Vec<f32>>;

/// reference src/tag_families.rs:5-13 -- the discriminants are `agx_family` (checked by tests/test_rust_binding.py).
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
#[repr(i32)]
pub enum TagFamily {
    T16H5 = 0,
    T25H7 = 1,
    T25H9 = 2,
    T36H11 = 3,
    /// 1 bit Border
    T36H11B1 = 4,
}

impl std::str::FromStr for TagFamily {
    type Err = std::fmt::Error;
    /// reference src/tag_families.rs:15-28, through `agx_family_from_str` (one table, the library's).
    fn from_str(s: &str) -> Result<Self, Self::Err> {
        let name = std::ffi::CString::new(s).map_err(|_| std::fmt::Error)?;
        let mut fam: c_int = -1;
        let st = unsafe { ffi::agx_family_from_str(name.as_ptr(), &mut fam) };
        match (st, fam) {
            (ffi::AGX_OK, ffi::AGX_T16H5) => Ok(TagFamily::T16H5),
            (ffi::AGX_OK, ffi::AGX_T25H7) => Ok(TagFamily::T25H7),
            (ffi::AGX_OK, ffi::AGX_T25H9) => Ok(TagFamily::T25H9),
            (ffi::AGX_OK, ffi::AGX_T36H11) => Ok(TagFamily::T36H11),
            (ffi::AGX_OK, ffi::AGX_T36H11B1) => Ok(TagFamily::T36H11B1),
            _ => Err(std::fmt::Error),
        }
    }
}

/// reference src/detector.rs:25-41
#[derive(Debug, Clone, Copy)]
pub struct DetectorParams {
    pub tag_spacing_ratio: f32,
    pub min_saddle_angle: f32,
    pub max_saddle_angle: f32,
    pub max_num_of_boards: u8,
}

impl DetectorParams {
    pub fn default_params() -> DetectorParams {
        DetectorParams { tag_spacing_ratio: 0.3, min_saddle_angle: 30.0, max_saddle_angle: 60.0, max_num_of_boards: 2 }
    }
}

/// reference src/saddle.rs:3-15
#[derive(Debug, Clone, Copy)]
pub struct Saddle {
    pub p: (f32, f32),
    pub k: f32,
    pub theta: f32,
    pub phi: f32,
}

impl Saddle {
    pub const fn arr(&self) -> [f32; 2] {
        [self.p.0, self.p.1]
    }
}

/// What the ABI is handed for one image: borrowed pixels of a natively supported variant, or the two planes the
/// reference derives itself (src/detector.rs:409 `to_luma32f`, :507 `to_luma8`) for every other variant.
enum Input<'a> {
    Native { px: *const c_void, stride: usize, fmt: c_int, _keep: std::marker::PhantomData<&'a ()> },
    Planes { luma32f: image::ImageBuffer<image::Luma<f32>, Vec<f32>>, luma8: image::GrayImage },
}

/// A pooled handle; back in the pool when dropped -- also when the closure that used it panics (a handle owns about
/// 5 GB of device workspace at 256 frames of 1280 x 800 and must not leak).
struct Lease<'a> {
    pool: &'a Mutex<Vec<Handle>>,
    h: Option<Handle>,
}
impl Drop for Lease<'_> {
    fn drop(&mut self) {
        if let Some(h) = self.h.take() {
            match self.pool.lock() {
                Ok(mut p) => p.push(h),
                Err(_) => unsafe { ffi::agx_detector_destroy(h.0) },
            }
        }
    }
}

/// `*mut agx_detector` that may move between threads (a handle is one device + stream: used by one thread at a time,
/// which the pool guarantees).
struct Handle(*mut ffi::agx_detector);
unsafe impl Send for Handle {}

/// Same surface as `aprilgrid::detector::TagDetector`.  The reference's detector is `Send + Sync` and `detect(&self)`
/// may be called from any number of threads (src/detector.rs:17-23); here every call leases a handle from a pool
/// (created on demand), so the property holds.
pub struct TagDetector {
    pool: Mutex<Vec<Handle>>,
    family: c_int,
    params: ffi::agx_params,
    device: c_int,
    blur_sigma: Option<f32>,
    half_size_patch: Option<i32>,
}

impl TagDetector {
    /// reference src/detector.rs:364-406.  Infallible like the reference's: the device is touched by the first call.
    pub fn new(tag_family: &TagFamily, optional_detector_params: Option<DetectorParams>) -> TagDetector {
        Self::new_on_device(tag_family, optional_detector_params, 0)
    }

    /// The same on GPU `device` of the node (one `TagDetector` per GPU shards a stream of frames; frames are independent).
    pub fn new_on_device(tag_family: &TagFamily, optional_detector_params: Option<DetectorParams>, device: i32) -> TagDetector {
        let p = optional_detector_params.unwrap_or(DetectorParams::default_params());
        TagDetector {
            pool: Mutex::new(Vec::new()),
            family: *tag_family as c_int,
            device: device as c_int,
            params: ffi::agx_params {
                tag_spacing_ratio: p.tag_spacing_ratio,
                min_saddle_angle: p.min_saddle_angle,
                max_saddle_angle: p.max_saddle_angle,
                max_num_of_boards: p.max_num_of_boards,
            },
            blur_sigma: None,
            half_size_patch: None,
        }
    }

    /// The sigma of the chain's blur (the reference hard-codes 1.5 at src/detector.rs:410, the default): positive, finite,
    /// at most 8.  Applied to every pooled handle when it is created; a sigma the library refuses panics there, like a
    /// failed creation.  Handles that already exist are dropped, so the value holds from the next call on.
    pub fn with_blur_sigma(mut self, sigma: f32) -> TagDetector {
        self.blur_sigma = Some(sigma);
        for h in self.pool.get_mut().unwrap().drain(..) {
            unsafe { ffi::agx_detector_destroy(h.0) };
        }
        self
    }

    /// rochade_refine's half_size_patch inside the chain (the reference hard-codes 2 at src/detector.rs:430, the default):
    /// 1 ..= 4.  Applied like `with_blur_sigma`: to every pooled handle when it is created, a refused value panics there, and
    /// handles that already exist are dropped.
    pub fn with_half_size_patch(mut self, half_size_patch: i32) -> TagDetector {
        self.half_size_patch = Some(half_size_patch);
        for h in self.pool.get_mut().unwrap().drain(..) {
            unsafe { ffi::agx_detector_destroy(h.0) };
        }
        self
    }

    fn with_handle<R>(&self, f: impl FnOnce(*mut ffi::agx_detector) -> R) -> R {
        let pooled = self.pool.lock().unwrap().pop();
        let h = pooled.unwrap_or_else(|| {
            let mut h: *mut ffi::agx_detector = std::ptr::null_mut();
            let st = unsafe { ffi::agx_detector_create(self.family, &self.params, self.device, &mut h) };
            assert_eq!(st, ffi::AGX_OK, "agx_detector_create failed: {} ({})", st, last_error(std::ptr::null()));
            if let Some(sigma) = self.blur_sigma {
                let st = unsafe { ffi::agx_detector_set_blur_sigma(h, sigma) };
                assert_eq!(st, ffi::AGX_OK, "agx_detector_set_blur_sigma({}) failed: {} ({})", sigma, st, last_error(h));
            }
            if let Some(half) = self.half_size_patch {
                let st = unsafe { ffi::agx_detector_set_half_size_patch(h, half) };
                assert_eq!(st, ffi::AGX_OK, "agx_detector_set_half_size_patch({}) failed: {} ({})", half, st, last_error(h));
            }
            Handle(h)
        });
        let lease = Lease { pool: &self.pool, h: Some(h) };
        f(lease.h.as_ref().unwrap().0)
    }

    fn input(img: &image::DynamicImage) -> (Input<'_>, u32, u32) {
        use image::DynamicImage::*;
        let native = |px: *const c_void, stride: usize, fmt: c_int| Input::Native { px, stride, fmt, _keep: std::marker::PhantomData };
        match img {
            // the three variants the reference's tests, benches and detect_kornia feed the path: no copy, the luma
            // conversion is fused into the blur kernel's load stage
            ImageLuma8(b) => (native(b.as_raw().as_ptr() as *const c_void, b.width() as usize, ffi::AGX_L8), b.width(), b.height()),
            ImageLuma16(b) => (native(b.as_raw().as_ptr() as *const c_void, 2 * b.width() as usize, ffi::AGX_L16), b.width(), b.height()),
            ImageRgb8(b) => (native(b.as_raw().as_ptr() as *const c_void, 3 * b.width() as usize, ffi::AGX_RGB8), b.width(), b.height()),
            // the other integer variants: no copy either, the library's front-end kernel writes their integer luma plane
            // and the L8 / L16 chain reads that (alpha dropped; (2126 R + 7152 G + 722 B) / 10000, the image crate's own)
            ImageLumaA8(b) => (native(b.as_raw().as_ptr() as *const c_void, 2 * b.width() as usize, ffi::AGX_LA8), b.width(), b.height()),
            ImageRgba8(b) => (native(b.as_raw().as_ptr() as *const c_void, 4 * b.width() as usize, ffi::AGX_RGBA8), b.width(), b.height()),
            ImageLumaA16(b) => (native(b.as_raw().as_ptr() as *const c_void, 4 * b.width() as usize, ffi::AGX_LA16), b.width(), b.height()),
            ImageRgb16(b) => (native(b.as_raw().as_ptr() as *const c_void, 6 * b.width() as usize, ffi::AGX_RGB16), b.width(), b.height()),
            ImageRgba16(b) => (native(b.as_raw().as_ptr() as *const c_void, 8 * b.width() as usize, ffi::AGX_RGBA16), b.width(), b.height()),
            // Rgb32F, Rgba32F (and variants a later image crate adds): exactly the planes the reference computes
            other => (Input::Planes { luma32f: other.to_luma32f(), luma8: other.to_luma8() }, other.width(), other.height()),
        }
    }

    /// reference src/detector.rs:408-446 -- the hot path.
    pub fn refined_saddle_points(&self, img: &image::DynamicImage) -> Vec<Saddle> {
        let (inp, w, h) = Self::input(img);
        let (px, stride, fmt) = match &inp {
            Input::Native { px, stride, fmt, .. } => (*px, *stride, *fmt),
            Input::Planes { luma32f, .. } => (luma32f.as_raw().as_ptr() as *const c_void, 4 * w as usize, ffi::AGX_LF32),
        };
        let mut out = vec![ffi::agx_saddle::default(); 4096];
        let mut n = 0u32;
        let call = |out: &mut Vec<ffi::agx_saddle>, n: &mut u32| {
            self.with_handle(|d| unsafe {
                ffi::agx_refined_saddle_points(d, px, w as c_int, h as c_int, stride, fmt, out.as_mut_ptr(), out.len() as u32, n)
            })
        };
        let mut st = call(&mut out, &mut n);
        if st == ffi::AGX_ERR_CAPACITY && n as usize > out.len() {
            // Vec<Saddle> has no limit: the call reported the size it needs
            out.resize(n as usize, ffi::agx_saddle::default());
            st = call(&mut out, &mut n);
        }
        assert_eq!(st, ffi::AGX_OK, "agx_refined_saddle_points failed: {}", st);
        out[..n as usize].iter().map(|s| Saddle { p: (s.x, s.y), k: s.k, theta: s.theta, phi: s.phi }).collect()
    }

    /// reference src/detector.rs:194-361, `rochade_refine(image_input, initial_corners, 2)` with `image_input` the sigma = 1.5
    /// blur of `img`, as `refined_saddle_points` feeds it (:409-410, :430): the refined corners, in input order.
    pub fn rochade_refine(&self, img: &image::DynamicImage, initial_corners: &[(f32, f32)]) -> Vec<Saddle> {
        let (records, status) = self.rochade_refine_with_status(img, initial_corners);
        records.into_iter().zip(status).filter(|(_, st)| *st == ffi::AGX_POINT_REFINED as u32).map(|(s, _)| s).collect()
    }

    /// The same with an answer for every corner: its record (zeros unless refined) and why it was kept or dropped
    /// (`AGX_POINT_REFINED`, `_OUTSIDE`, `_NOT_SADDLE`, `_MOVED`), in input order.
    pub fn rochade_refine_with_status(&self, img: &image::DynamicImage, initial_corners: &[(f32, f32)]) -> (Vec<Saddle>, Vec<u32>) {
        self.rochade_refine_h_with_status(img, initial_corners, 2)
    }

    /// reference src/detector.rs:194-361, `rochade_refine(image_input, initial_corners, half_size_patch)` with the crate's third
    /// argument, 1 ..= 4: the refined corners, in input order.  `rochade_refine` is this at 2, what the detector passes (:430).
    pub fn rochade_refine_h(&self, img: &image::DynamicImage, initial_corners: &[(f32, f32)], half_size_patch: i32) -> Vec<Saddle> {
        let (records, status) = self.rochade_refine_h_with_status(img, initial_corners, half_size_patch);
        records.into_iter().zip(status).filter(|(_, st)| *st == ffi::AGX_POINT_REFINED as u32).map(|(s, _)| s).collect()
    }

    /// The same with an answer for every corner, as `rochade_refine_with_status`.
    pub fn rochade_refine_h_with_status(&self, img: &image::DynamicImage, initial_corners: &[(f32, f32)], half_size_patch: i32) -> (Vec<Saddle>, Vec<u32>) {
        let (inp, w, h) = Self::input(img);
        let (px, stride, fmt) = match &inp {
            Input::Native { px, stride, fmt, .. } => (*px, *stride, *fmt),
            Input::Planes { luma32f, .. } => (luma32f.as_raw().as_ptr() as *const c_void, 4 * w as usize, ffi::AGX_LF32),
        };
        let points: Vec<ffi::agx_point> = initial_corners.iter().map(|p| ffi::agx_point { x: p.0, y: p.1 }).collect();
        let mut out = vec![ffi::agx_saddle::default(); points.len()];
        let mut status = vec![0u32; points.len()];
        let mut n_refined = 0u32;
        let st = self.with_handle(|d| unsafe {
            ffi::agx_rochade_refine_h(
                d, px, w as c_int, h as c_int, stride, fmt, ffi::AGX_REFINE_BLURRED, points.as_ptr() as *const c_void,
                points.len() as u32, out.as_mut_ptr(), status.as_mut_ptr(), &mut n_refined, half_size_patch as c_int,
            )
        });
        assert_eq!(st, ffi::AGX_OK, "agx_rochade_refine_h failed: {}", st);
        (out.iter().map(|s| Saddle { p: (s.x, s.y), k: s.k, theta: s.theta, phi: s.phi }).collect(), status)
    }

    /// reference src/image_util.rs:110-206, `gaussian_blur_f32(img, sigma)`: the blur of an f32 luma plane at any sigma with
    /// `ceil(2 sigma)` in 1 ..= 16, bit for bit.
    pub fn gaussian_blur_f32(&self, img: &GrayImagef32, sigma: f32) -> GrayImagef32 {
        let (w, h) = (img.width(), img.height());
        let mut out = vec![0f32; w as usize * h as usize];
        let st = self.with_handle(|d| unsafe {
            ffi::agx_gaussian_blur_f32(
                d, img.as_raw().as_ptr() as *const c_void, w as c_int, h as c_int, 4 * w as usize, ffi::AGX_LF32, sigma, out.as_mut_ptr(),
            )
        });
        assert_eq!(st, ffi::AGX_OK, "agx_gaussian_blur_f32 failed: {}", st);
        GrayImagef32::from_raw(w, h, out).unwrap()
    }

    /// reference src/image_util.rs:72-109, `hessian_response(img)`: the Hessian determinant of an f32 plane (the border ring is 0).
    pub fn hessian_response(&self, img: &GrayImagef32) -> GrayImagef32 {
        let (w, h) = (img.width(), img.height());
        let mut out = vec![0f32; w as usize * h as usize];
        let st = self.with_handle(|d| unsafe {
            ffi::agx_hessian_response(d, img.as_raw().as_ptr() as *const c_void, w as c_int, h as c_int, 4 * w as usize, ffi::AGX_LF32, out.as_mut_ptr())
        });
        assert_eq!(st, ffi::AGX_OK, "agx_hessian_response failed: {}", st);
        GrayImagef32::from_raw(w, h, out).unwrap()
    }

    /// reference src/detector.rs:414-429 on a response plane of the caller's: the frame minimum, the threshold `0.05 * min`,
    /// `init_saddle_clusters` and the centroid map.  `Some(centres)` in the reference's order; `None` where the plane is refused
    /// (a pixel of its outermost ring is below the threshold, AGX_CLUSTERS_BORDER) or holds more than 16384 clusters.
    pub fn cluster_centers(&self, response: &GrayImagef32) -> Option<Vec<(f32, f32)>> {
        let (w, h) = (response.width(), response.height());
        let cap = 16384u32;
        let mut rows: Vec<ffi::agx_cluster_info> = Vec::with_capacity(cap as usize);
        let (mut n, mut status) = (0u32, 0u32);
        let st = self.with_handle(|d| unsafe {
            ffi::agx_cluster_centers(d, response.as_raw().as_ptr(), w as c_int, h as c_int, 4 * w as usize, rows.as_mut_ptr(), cap, &mut n, &mut status)
        });
        assert_eq!(st, ffi::AGX_OK, "agx_cluster_centers failed: {}", st);
        if (status & 0xff) as c_int != ffi::AGX_CLUSTERS_OK {
            return None;
        }
        unsafe { rows.set_len(n as usize) };
        Some(rows.iter().map(|c| (c.cx, c.cy)).collect())
    }

    /// reference src/detector.rs:448-476, `try_decode_quad(&self, img, quad)` for every quad of `quads` (the crate's pub fns
    /// `decode_positions`, `bit_code`, `best_tag` and the corner rotation of :467-470), on `img.to_luma8()`; the board search is
    /// not run.  `Some((id, corners))` where the reference returns `Some`, in input order.
    pub fn decode_quads(&self, img: &image::DynamicImage, quads: &[[(f32, f32); 4]]) -> Vec<Option<(u32, [(f32, f32); 4])>> {
        self.decode_quads_with_status(img, quads).0
    }

    /// The same with the reason for every `None` (`AGX_QUAD_OUTSIDE`, `_LOW_CONTRAST`, `_AMBIGUOUS`, `_NO_MATCH`; a corner that is
    /// not finite is `AGX_QUAD_OUTSIDE`) and `bit_code`'s value where there is one, in input order.
    pub fn decode_quads_with_status(&self, img: &image::DynamicImage, quads: &[[(f32, f32); 4]]) -> (Vec<Option<(u32, [(f32, f32); 4])>>, Vec<u32>, Vec<u64>) {
        let (inp, w, h) = Self::input(img);
        let (px, stride, fmt) = match &inp {
            Input::Native { px, stride, fmt, .. } => (*px, *stride, *fmt),
            Input::Planes { luma8, .. } => (luma8.as_raw().as_ptr() as *const c_void, w as usize, ffi::AGX_L8),
        };
        let flat: Vec<f32> = quads.iter().flat_map(|q| q.iter().flat_map(|p| [p.0, p.1])).collect();
        let mut out = vec![ffi::agx_tag { id: 0, xy: [0.0; 8] }; quads.len()];
        let mut status = vec![0u32; quads.len()];
        let mut bits = vec![0u64; quads.len()];
        let mut n_decoded = 0u32;
        let st = self.with_handle(|d| unsafe {
            ffi::agx_decode_quads(
                d, px, w as c_int, h as c_int, stride, fmt, flat.as_ptr() as *const c_void, quads.len() as u32, out.as_mut_ptr(),
                status.as_mut_ptr(), bits.as_mut_ptr(), &mut n_decoded,
            )
        });
        assert_eq!(st, ffi::AGX_OK, "agx_decode_quads failed: {}", st);
        let tags = out
            .iter()
            .zip(&status)
            .map(|(t, s)| {
                if *s == ffi::AGX_QUAD_DECODED as u32 {
                    Some((t.id, [(t.xy[0], t.xy[1]), (t.xy[2], t.xy[3]), (t.xy[4], t.xy[5]), (t.xy[6], t.xy[7])]))
                } else {
                    None
                }
            })
            .collect();
        (tags, status, bits)
    }

    fn tags_to_map(out: &[ffi::agx_tag]) -> HashMap<u32, [(f32, f32); 4]> {
        // later entries replace earlier ones, as HashMap::insert does at src/detector.rs:520
        out.iter().map(|t| (t.id, [(t.xy[0], t.xy[1]), (t.xy[2], t.xy[3]), (t.xy[4], t.xy[5]), (t.xy[6], t.xy[7])])).collect()
    }

    /// reference src/detector.rs:505-540
    pub fn detect(&self, img: &image::DynamicImage) -> HashMap<u32, [(f32, f32); 4]> {
        let (inp, w, h) = Self::input(img);
        let mut out = vec![ffi::agx_tag { id: 0, xy: [0.0; 8] }; 1024];
        let mut n = 0u32;
        let st = self.with_handle(|d| unsafe {
            match &inp {
                Input::Native { px, stride, fmt, .. } => {
                    ffi::agx_detect(d, *px, w as c_int, h as c_int, *stride, *fmt, out.as_mut_ptr(), out.len() as u32, &mut n)
                }
                Input::Planes { luma32f, luma8 } => ffi::agx_detect_planes(
                    d, luma32f.as_raw().as_ptr(), 4 * w as usize, luma8.as_raw().as_ptr(), w as usize, w as c_int, h as c_int,
                    out.as_mut_ptr(), out.len() as u32, &mut n,
                ),
            }
        });
        assert_eq!(st, ffi::AGX_OK, "agx_detect failed: {}", st);
        Self::tags_to_map(&out[..n as usize])
    }

    /// reference src/detector.rs:478-503: `kornia::image::Image<u8, N>`, N = 1 (u8c1) or 3 (u8c3, HWC interleaved), and
    /// beyond the reference N = 4 (u8c4 as R,G,B,A: `AGX_RGBA8`); any other N panics with the reference's message.  The tensor's storage is handed over as it is (the reference
    /// clones it into a GrayImage / RgbImage first).
    #[cfg(feature = "kornia")]
    pub fn detect_kornia<const N: usize>(&self, img: &kornia::image::Image<u8, N>) -> HashMap<u32, [(f32, f32); 4]> {
        let fmt = match img.num_channels() {
            1 => ffi::AGX_L8,
            3 => ffi::AGX_RGB8,
            4 => ffi::AGX_RGBA8,
            _ => panic!("Only support u8c1 and u8c3"),
        };
        let (w, h) = (img.width(), img.height());
        let px: &[u8] = img.as_slice(); // H x W x N, row-major, tightly packed
        debug_assert_eq!(px.len(), w * h * N);
        let mut out = vec![ffi::agx_tag { id: 0, xy: [0.0; 8] }; 1024];
        let mut n = 0u32;
        let st = self.with_handle(|d| unsafe {
            ffi::agx_detect(d, px.as_ptr() as *const c_void, w as c_int, h as c_int, N * w, fmt, out.as_mut_ptr(), out.len() as u32, &mut n)
        });
        assert_eq!(st, ffi::AGX_OK, "agx_detect failed: {}", st);
        Self::tags_to_map(&out[..n as usize])
    }

    /// `detect` of every frame of a tightly packed `[n][h][w]` u8 buffer (no counterpart in the reference).  Upload,
    /// saddle chain, board search and decode run chunk by chunk on the device (`agx_detect_batch`; frames the device
    /// cannot decide take the same search on a pool of host threads, 0 = every CPU the process is granted).  The maps
    /// are those of calling `detect` per frame.
    pub fn detect_many(&self, frames: &[u8], n: usize, w: u32, h: u32) -> Vec<HashMap<u32, [(f32, f32); 4]>> {
        assert_eq!(frames.len(), n * (w as usize) * (h as usize));
        const CAP: usize = 256;
        let mut out = vec![ffi::agx_tag { id: 0, xy: [0.0; 8] }; n * CAP];
        let mut counts = vec![0u32; n];
        let mut status = vec![0 as c_int; n];
        let st = self.with_handle(|d| unsafe {
            ffi::agx_detect_batch(
                d, frames.as_ptr() as *const c_void, std::ptr::null(), n as c_int, w as c_int, h as c_int, w as usize,
                (w as usize) * (h as usize), ffi::AGX_L8, out.as_mut_ptr(), CAP as u32, counts.as_mut_ptr(), status.as_mut_ptr(), 0,
            )
        });
        assert_eq!(st, ffi::AGX_OK, "agx_detect_batch failed: {}", st);
        (0..n).map(|i| Self::tags_to_map(&out[i * CAP..i * CAP + counts[i] as usize])).collect()
    }
}

impl Drop for TagDetector {
    fn drop(&mut self) {
        let handles = match self.pool.lock() {
            Ok(mut p) => std::mem::take(&mut *p),
            Err(e) => std::mem::take(&mut *e.into_inner()),
        };
        for h in handles {
            unsafe { ffi::agx_detector_destroy(h.0) }
        }
    }
}

/// reference src/detector.rs:588-639, `try_find_best_board(refined: &[Saddle]) -> Option<Vec<[usize; 4]>>`: the quads of the
/// best board in a saddle list, as indices into `refined`, in the reference's order.  The host form (no device is used).
/// Panics on a saddle whose x, y or theta is not finite, as the reference does on such coordinates (:594).
pub fn find_best_board(refined: &[Saddle]) -> Option<Vec<[usize; 4]>> {
    let list: Vec<ffi::agx_saddle> =
        refined.iter().map(|s| ffi::agx_saddle { x: s.p.0, y: s.p.1, k: s.k, theta: s.theta, phi: s.phi }).collect();
    let mut cap = 128u32;
    loop {
        let mut quads = vec![0u32; cap as usize * 4];
        let (mut n, mut status) = (0u32, 0u32);
        let st = unsafe { ffi::agx_find_board_tail(list.as_ptr(), list.len() as u32, quads.as_mut_ptr(), cap, &mut n, &mut status) };
        assert_eq!(st, ffi::AGX_OK, "agx_find_board_tail failed: {}", st);
        match status as c_int {
            ffi::AGX_BOARD_FOUND => {
                return Some(quads[..n as usize * 4].chunks(4).map(|q| [q[0] as usize, q[1] as usize, q[2] as usize, q[3] as usize]).collect())
            }
            ffi::AGX_BOARD_CAPACITY => cap = n,
            ffi::AGX_BOARD_NONE => return None,
            _ => panic!("find_best_board: a saddle's x, y or theta is not finite"),
        }
    }
}

/// reference src/detector.rs:543-586, `init_quads(refined, s0_idx, tree)`, for every seed in order: the candidate quads of each
/// seed saddle as indices into `refined`, in the reference's loop and corner order, among the `n_nearest` (2 ..= 64; the
/// reference's is 50) nearest saddles of the seed.  `seeds = None`: try_find_best_board's own seeds (:601-616), at most
/// `max_seeds` of them (the reference takes 30).  Returns `(quads, quads per seed, the seeds taken)`.  The host form (no device is
/// used).  Panics on a saddle whose x, y or theta is not finite, on a seed index beyond the list and on an `n_nearest` outside
/// 2 ..= 64.
pub fn init_quads_tail(refined: &[Saddle], seeds: Option<&[usize]>, max_seeds: usize, n_nearest: u32) -> (Vec<[usize; 4]>, Vec<u32>, Vec<usize>) {
    let list: Vec<ffi::agx_saddle> =
        refined.iter().map(|s| ffi::agx_saddle { x: s.p.0, y: s.p.1, k: s.k, theta: s.theta, phi: s.phi }).collect();
    let given: Option<Vec<u32>> = seeds.map(|s| s.iter().map(|&i| i as u32).collect());
    let room = match &given {
        Some(s) => s.len().max(1),
        None => max_seeds.max(1),
    };
    let no_seed = [0u32; 1];  // (a non-null pointer for an empty seed list: null asks for the reference's seeds)
    let (seed_ptr, n_seeds) = match &given {
        Some(s) if !s.is_empty() => (s.as_ptr(), s.len() as u32),
        Some(_) => (no_seed.as_ptr(), 0u32),
        None => (std::ptr::null(), 0u32),
    };
    let mut cap = 1024u32;
    loop {
        let mut quads = vec![0u32; cap as usize * 4];
        let mut counts = vec![0u32; room];
        let mut taken = vec![0u32; room];
        let (mut n, mut status, mut n_taken) = (0u32, 0u32, 0u32);
        let st = unsafe {
            ffi::agx_init_quads_tail(list.as_ptr(), list.len() as u32, std::ptr::null(), seed_ptr, n_seeds, room as u32, n_nearest,
                                     quads.as_mut_ptr(), cap, &mut n, &mut status, counts.as_mut_ptr(), taken.as_mut_ptr(), &mut n_taken)
        };
        assert_eq!(st, ffi::AGX_OK, "agx_init_quads_tail failed: {}", st);
        counts.truncate(n_taken as usize);
        let taken: Vec<usize> = taken[..n_taken as usize].iter().map(|&s| s as usize).collect();
        match status as c_int {
            ffi::AGX_BOARD_FOUND => {
                let rows = quads[..n as usize * 4].chunks(4).map(|q| [q[0] as usize, q[1] as usize, q[2] as usize, q[3] as usize]).collect();
                return (rows, counts, taken);
            }
            ffi::AGX_BOARD_CAPACITY => cap = n,
            ffi::AGX_BOARD_NONE => return (Vec::new(), counts, taken),
            _ => panic!("init_quads_tail: a saddle's x, y or theta is not finite, or a seed names no saddle of the list"),
        }
    }
}

/// reference src/board.rs:26-112 as try_find_best_board uses it (src/detector.rs:613-633), for a caller who already knows quads of
/// the board: `Board::new(refined, all-true mask, seed, spacing_ratio, tree)` for every seed in order, the first one whose score is
/// strictly above every earlier one, `try_fix_missing` on it if `fix_missing`, then `all_tag_indexes`.  `stop_score > 0` ends the
/// loop behind the first seed that leaves the best score at or above it (the caller's rule, not the reference's `>= 36` per seed
/// saddle).  Returns `(quads, score of every seed, index of the chosen seed)`, or `None` without a seed.  The host form (no
/// device is used).  Panics on a saddle whose x, y or theta is not finite, on a seed index beyond the list and on a
/// `spacing_ratio` that is not finite or at or below -1.
pub fn grow_board_tail(refined: &[Saddle], seeds: &[[usize; 4]], spacing_ratio: f32, stop_score: u32, fix_missing: bool)
                       -> Option<(Vec<[usize; 4]>, Vec<u32>, usize)> {
    let list: Vec<ffi::agx_saddle> =
        refined.iter().map(|s| ffi::agx_saddle { x: s.p.0, y: s.p.1, k: s.k, theta: s.theta, phi: s.phi }).collect();
    let seed_rows: Vec<u32> = seeds.iter().flat_map(|q| q.iter().map(|&i| i as u32)).collect();
    let flags = if fix_missing { ffi::AGX_GROW_FIX_MISSING } else { 0 };
    let mut cap = 128u32;
    loop {
        let mut quads = vec![0u32; cap as usize * 4];
        let mut scores = vec![0u32; seeds.len()];
        let (mut n, mut status, mut best) = (0u32, 0u32, 0u32);
        let st = unsafe {
            ffi::agx_grow_board_tail(list.as_ptr(), list.len() as u32, std::ptr::null(), seed_rows.as_ptr(), seeds.len() as u32, spacing_ratio,
                                     stop_score, flags, quads.as_mut_ptr(), cap, &mut n, &mut status, scores.as_mut_ptr(), &mut best)
        };
        assert_eq!(st, ffi::AGX_OK, "agx_grow_board_tail failed: {}", st);
        match status as c_int {
            ffi::AGX_BOARD_FOUND => {
                let rows = quads[..n as usize * 4].chunks(4).map(|q| [q[0] as usize, q[1] as usize, q[2] as usize, q[3] as usize]).collect();
                return Some((rows, scores, best as usize));
            }
            ffi::AGX_BOARD_CAPACITY => cap = n,
            ffi::AGX_BOARD_NONE => return None,
            _ => panic!("grow_board_tail: a saddle's x, y or theta is not finite, or a seed names no saddle of the list"),
        }
    }
}

/// Corners known from an earlier frame snapped to this frame's saddles: every point of every row (`N` = 1..=4 points a row) to the
/// nearest saddle of `refined` by `kdtree::distance::squared_euclidean` in `f32` (reference src/detector.rs:15), the lowest index
/// at equal distance, taken if the squared distance is at most `max_dist_sq`; `reverse` reads a row back to front (a tag's
/// corners, src/detector.rs:467-470, are then a quad in `init_quads`' winding).  Returns `(slots, rows)`: per row and point the
/// saddle index or `None`, and `(row, indices)` of the rows whose points all snapped to pairwise distinct saddles, in row order --
/// with `N` = 4 the seeds of `grow_board_tail`.  The host form (no device is used).  Panics on a saddle whose x or y is not finite
/// and on a `max_dist_sq` that is negative or NaN.
pub fn snap_points_tail<const N: usize>(refined: &[Saddle], rows: &[[(f32, f32); N]], max_dist_sq: f32, reverse: bool)
                                        -> (Vec<[Option<usize>; N]>, Vec<(usize, [usize; N])>) {
    assert!((1..=4).contains(&N), "snap_points_tail: 1 to 4 points a row");
    let list: Vec<ffi::agx_saddle> =
        refined.iter().map(|s| ffi::agx_saddle { x: s.p.0, y: s.p.1, k: s.k, theta: s.theta, phi: s.phi }).collect();
    let flat: Vec<f32> = rows.iter().flat_map(|r| r.iter().flat_map(|p| [p.0, p.1])).collect();
    let mut slots = vec![0u32; (rows.len() * N).max(1)];
    let mut kept = vec![0u32; (rows.len() * N).max(1)];
    let mut index = vec![0u32; rows.len().max(1)];
    let (mut n_kept, mut status) = (0u32, 0u32);
    let st = unsafe {
        ffi::agx_snap_points_tail(list.as_ptr(), list.len() as u32, std::ptr::null(), flat.as_ptr() as *const c_void, 8 * N, 8, rows.len() as u32,
                                  N as u32, max_dist_sq, if reverse { ffi::AGX_SNAP_REVERSE } else { 0 }, slots.as_mut_ptr(),
                                  std::ptr::null_mut(), kept.as_mut_ptr(), &mut n_kept, index.as_mut_ptr(), &mut status)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_snap_points_tail failed: {}", st);
    assert_eq!(status as c_int, ffi::AGX_SNAP_OK, "snap_points_tail: a saddle's x or y is not finite");
    let per_point = |v: u32| if v == ffi::AGX_SNAP_NONE { None } else { Some(v as usize) };
    let all: Vec<[Option<usize>; N]> = (0..rows.len()).map(|r| std::array::from_fn(|p| per_point(slots[r * N + p]))).collect();
    let whole = (0..n_kept as usize).map(|k| (index[k] as usize, std::array::from_fn(|p| kept[k * N + p] as usize))).collect();
    (all, whole)
}

/// reference src/detector.rs:42-72, `decode_positions`: the sample points of a quad (four corners), x outer and y inner, or
/// `None` where a rounded corner lies outside the image.  The host form (no device is used).  A corner that is not finite is
/// `None`.  Panics where the library refuses the arguments: `edge_bits` outside 1..=8, `border_bits` above 16, a margin that
/// is not finite or a source square that is a point, or a quad that does not have four corners.
pub fn decode_positions(img_w: u32, img_h: u32, quad_pts: &[(f32, f32)], border_bits: u8, edge_bits: u8, margin: f32) -> Option<Vec<(f32, f32)>> {
    assert_eq!(quad_pts.len(), 4, "decode_positions: a quad has four corners");
    let flat: Vec<f32> = quad_pts.iter().flat_map(|p| [p.0, p.1]).collect();
    let n = edge_bits as usize * edge_bits as usize;
    let mut points = vec![0f32; 2 * n.max(1)];
    let mut status = 0u32;
    let st = unsafe {
        ffi::agx_decode_positions_tail(flat.as_ptr() as *const c_void, 1, img_w, img_h, border_bits as c_int, edge_bits as c_int, margin,
                                       points.as_mut_ptr(), &mut status)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_decode_positions_tail failed: {}", st);
    if status as c_int != ffi::AGX_QUAD_DECODED {
        return None;
    }
    Some(points[..2 * n].chunks(2).map(|p| (p[0], p[1])).collect())
}

/// The sampling model of `decode_positions`: `tag_affine` (reference src/image_util.rs:39-70, what src/detector.rs:58 calls) or
/// `tag_homography` (src/image_util.rs:5-37).
#[repr(i32)]
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum TagMap {
    Affine = 0,
    Homography = 1,
}

/// `decode_positions` (reference src/detector.rs:42-72) with the map of :58 chosen by `model`.  `Err(status)` carries the reason
/// for `None` (`AGX_QUAD_OUTSIDE`, or `AGX_QUAD_DEGENERATE` where the homography refuses the quad).  Panics as `decode_positions`.
pub fn decode_positions_m(img_w: u32, img_h: u32, quad_pts: &[(f32, f32)], border_bits: u8, edge_bits: u8, margin: f32,
                          model: TagMap) -> Result<Vec<(f32, f32)>, u32> {
    assert_eq!(quad_pts.len(), 4, "decode_positions_m: a quad has four corners");
    let flat: Vec<f32> = quad_pts.iter().flat_map(|p| [p.0, p.1]).collect();
    let n = edge_bits as usize * edge_bits as usize;
    let mut points = vec![0f32; 2 * n.max(1)];
    let mut status = 0u32;
    let st = unsafe {
        ffi::agx_decode_positions_tail_m(flat.as_ptr() as *const c_void, 1, img_w, img_h, border_bits as c_int, edge_bits as c_int, margin,
                                         points.as_mut_ptr(), &mut status, model as c_int)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_decode_positions_tail_m failed: {}", st);
    if status as c_int != ffi::AGX_QUAD_DECODED {
        return Err(status);
    }
    Ok(points[..2 * n].chunks(2).map(|p| (p[0], p[1])).collect())
}

/// `tag_affine` / `tag_homography` (reference src/image_util.rs:39-70, :5-37) of quads of four corners each: the row-major 3 x 3
/// map from the source square of `side_bits` and `margin` to the image per quad, or `Err(status)` (`AGX_QUAD_OUTSIDE`: a corner
/// that is not finite; `AGX_QUAD_DEGENERATE`).  The host form.  Panics where the library refuses the arguments: `side_bits`
/// outside 1..=40, a margin that is not finite, a source square that is a point.
pub fn tag_maps_tail(quads: &[[(f32, f32); 4]], side_bits: u8, margin: f32, model: TagMap) -> Vec<Result<[f32; 9], u32>> {
    let flat: Vec<f32> = quads.iter().flat_map(|q| q.iter().flat_map(|p| [p.0, p.1])).collect();
    let mut maps = vec![0f32; 9 * quads.len().max(1)];
    let mut status = vec![0u32; quads.len().max(1)];
    let st = unsafe {
        ffi::agx_tag_maps_tail(flat.as_ptr() as *const c_void, quads.len() as u32, side_bits as c_int, margin, model as c_int,
                               maps.as_mut_ptr(), status.as_mut_ptr())
    };
    assert_eq!(st, ffi::AGX_OK, "agx_tag_maps_tail failed: {}", st);
    (0..quads.len())
        .map(|i| {
            if status[i] as c_int != ffi::AGX_QUAD_DECODED {
                return Err(status[i]);
            }
            let mut m = [0f32; 9];
            m.copy_from_slice(&maps[9 * i..9 * i + 9]);
            Ok(m)
        })
        .collect()
}

/// reference src/image_util.rs:5-37, `tag_homography`: the projective map from the tag's corner grid onto `quad_pts`, row-major,
/// scaled so that w is 1 at the grid's centre (the reference's vector has unit norm and an arbitrary sign); `None` where there
/// is no such map or the quad is not strictly convex.
pub fn tag_homography(quad_pts: &[(f32, f32)], side_bits: u8, margin: f32) -> Option<[f32; 9]> {
    assert_eq!(quad_pts.len(), 4, "tag_homography: a quad has four corners");
    let q = [quad_pts[0], quad_pts[1], quad_pts[2], quad_pts[3]];
    tag_maps_tail(&[q], side_bits, margin, TagMap::Homography)[0].ok()
}

/// reference src/detector.rs:74-122, `bit_code`: the bits of up to 64 sample points on a grey image, the first point the most
/// significant, or `None` (a point outside the image, too little contrast, too many samples near the mid brightness).  The
/// host form (no device is used).  A coordinate that is not finite is `None`.
pub fn bit_code(img: &image::GrayImage, decode_pts: &[(f32, f32)], valid_brightness_threshold: u8, max_invalid_bit: u32) -> Option<u64> {
    assert!(!decode_pts.is_empty() && decode_pts.len() <= 64, "bit_code: 1 to 64 points");
    let flat: Vec<f32> = decode_pts.iter().flat_map(|p| [p.0, p.1]).collect();
    let (mut bits, mut status) = (0u64, 0u32);
    let st = unsafe {
        ffi::agx_bit_code_tail(img.as_raw().as_ptr(), img.width() as c_int, img.height() as c_int, img.width() as usize, flat.as_ptr(),
                               decode_pts.len() as u32, 1, std::ptr::null(), valid_brightness_threshold as c_int, max_invalid_bit, &mut bits,
                               &mut status)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_bit_code_tail failed: {}", st);
    if status as c_int == ffi::AGX_QUAD_DECODED { Some(bits) } else { None }
}

/// reference src/detector.rs:142-169, `best_tag`: `(index into tag_family, rotation)` of the first rotation that lies within
/// `thres` of a code -- per rotation the first code with the smallest distance --, or `None`.  The host form (no device is
/// used).  `tag_family` holds 1 to 65535 codes.
pub fn best_tag(bits: u64, thres: u8, tag_family: &[u64], edge_bits: u8) -> Option<(usize, usize)> {
    assert!(!tag_family.is_empty() && tag_family.len() <= 65535, "best_tag: 1 to 65535 codes");
    let (mut id, mut rotation, mut status) = (0u32, 0u32, 0u32);
    let st = unsafe {
        ffi::agx_best_tag_tail(&bits, 1, std::ptr::null(), thres as c_int, 0, tag_family.as_ptr(), tag_family.len() as u32, edge_bits as c_int,
                               std::ptr::null(), &mut id, &mut rotation, &mut status, std::ptr::null_mut())
    };
    assert_eq!(st, ffi::AGX_OK, "agx_best_tag_tail failed: {}", st);
    if status as c_int == ffi::AGX_QUAD_DECODED { Some((id as usize, rotation as usize)) } else { None }
}

/// One round of `detect`'s loop behind its board search and decode, reference src/detector.rs:510-539, on the host (no device is
/// used): every quad of `quads` (saddle indices, as `find_best_board` returns them) whose `quad_status` is `AGX_QUAD_DECODED`
/// inserts its `quad_tags` entry into `tags` -- a known id keeps its place and takes the new corners (:520) -- and, where
/// `point_status` is given (a word per saddle), marks its four saddles `AGX_POINT_USED` (:521-536).  `tag_cap` bounds `tags`.
/// Returns the frame's `AGX_TAGS_*` status; pass it back in as `tag_status` for the next round (a status other than
/// `AGX_TAGS_OK` is sticky: the round changes nothing).
pub fn collect_tags_tail(tag_family: &TagFamily, quads: &[[u32; 4]], board_status: u32, quad_tags: &[(u32, [(f32, f32); 4])],
                         quad_status: &[u32], point_status: Option<&mut [u32]>, tag_cap: usize,
                         tags: &mut Vec<(u32, [(f32, f32); 4])>, tag_status: u32) -> u32 {
    assert!(quad_tags.len() == quads.len() && quad_status.len() == quads.len(), "one tag and one status per quad");
    assert!(tag_cap > 0 && tags.len() <= tag_cap, "tag_cap must hold the table");
    let flat: Vec<u32> = quads.iter().flat_map(|q| q.iter().copied()).collect();
    let to_c = |t: &(u32, [(f32, f32); 4])| ffi::agx_tag {
        id: t.0,
        xy: [t.1[0].0, t.1[0].1, t.1[1].0, t.1[1].1, t.1[2].0, t.1[2].1, t.1[3].0, t.1[3].1],
    };
    let c_quad_tags: Vec<ffi::agx_tag> = quad_tags.iter().map(to_c).collect();
    let mut rows: Vec<ffi::agx_tag> = tags.iter().map(to_c).collect();
    rows.resize_with(tag_cap, || ffi::agx_tag { id: 0, xy: [0.0; 8] });
    let (mut n_tags, mut status) = (tags.len() as u32, tag_status);
    let (n_slots, words) = match point_status {
        Some(w) => (w.len() as u32, w.as_mut_ptr()),
        None => (u32::MAX, std::ptr::null_mut()),
    };
    let st = unsafe {
        ffi::agx_collect_tags_tail(*tag_family as c_int, quads.len() as u32, flat.as_ptr(), board_status, c_quad_tags.as_ptr(),
                                   quad_status.as_ptr(), n_slots, words, tag_cap as u32, rows.as_mut_ptr(), &mut n_tags, &mut status)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_collect_tags_tail failed: {}", st);
    if status as c_int == ffi::AGX_TAGS_OK {
        tags.clear();
        for r in &rows[..n_tags as usize] {
            tags.push((r.id, [(r.xy[0], r.xy[1]), (r.xy[2], r.xy[3]), (r.xy[4], r.xy[5]), (r.xy[6], r.xy[7])]));
        }
    }
    status
}

/// The layout of a printed board, Kalibr's AprilGrid: tag `first_id + r * cols + c` sits at column `c`, row `r`; corner `j` of
/// its corners is the board point `(c (1 + s) + (0,1,1,0)[j], r (1 + s) + (0,0,1,1)[j])` in units of the tag side,
/// `s = spacing_ratio`.
#[derive(Clone, Copy, Debug)]
pub struct BoardLayout {
    pub cols: u32,
    pub rows: u32,
    pub first_id: u32,
    pub spacing_ratio: f32,
}

/// What `board_fit_tail` found for one frame.
#[derive(Clone, Debug)]
pub struct BoardFit {
    /// `AGX_FIT_OK` or `AGX_FIT_LOOSE`
    pub status: u32,
    /// row major, board units -> pixels, w = 1 at the board's centre
    pub h: [f64; 9],
    /// per row of the table: `AGX_FIT_ROW_*` and the squared residual in pixels (not written for an off-board row: NaN)
    pub rows: Vec<(u32, f32)>,
    pub n_inliers: usize,
    pub rms: f32,
    /// predicted tags in id order: all of the layout, or under `predict_missing` those that are not inlier rows
    pub pred: Vec<(u32, [(f32, f32); 4])>,
}

/// The homography from the printed board to the image through every corner of a frame's tag table (what `detect` returns), with
/// rounds that drop the row of the largest residual while that is above `max_err_sq` (px^2) and fewer than `max_drop` rows went,
/// and the predicted corners of the layout's tags.  The host form (no device is used); the reference has no such function (its
/// README's open item "Robustness").  `Err(status)`: `AGX_FIT_FEW`, `AGX_FIT_SINGULAR` or `AGX_FIT_INPUT`.  Panics where the
/// library refuses the arguments.
pub fn board_fit_tail(tags: &[(u32, [(f32, f32); 4])], layout: &BoardLayout, img_w: u32, img_h: u32, max_err_sq: f32, max_drop: u32,
                      min_tags: u32, predict_missing: bool) -> Result<BoardFit, u32> {
    let table: Vec<ffi::agx_tag> = tags.iter().map(|t| ffi::agx_tag {
        id: t.0,
        xy: [t.1[0].0, t.1[0].1, t.1[1].0, t.1[1].1, t.1[2].0, t.1[2].1, t.1[3].0, t.1[3].1],
    }).collect();
    // (the library refuses such a layout; checked here before the prediction rows are allocated from it)
    assert!(layout.cols > 0 && layout.rows > 0 && layout.cols as u64 * layout.rows as u64 <= 4096, "board_fit_tail: rows * cols in 1..=4096");
    let n_board = layout.cols as usize * layout.rows as usize;
    let mut h = [0f64; 9];
    let mut err = vec![f32::NAN; tags.len().max(1)];
    let mut row_status = vec![0u32; tags.len().max(1)];
    let mut pred = vec![ffi::agx_tag { id: 0, xy: [0.0; 8] }; n_board];
    let (mut n_inliers, mut n_pred, mut status, mut rms) = (0u32, 0u32, 0u32, 0f32);
    let st = unsafe {
        ffi::agx_board_fit_tail(table.as_ptr(), table.len() as u32, table.len() as u32, ffi::AGX_TAGS_OK as u32, layout.cols, layout.rows,
                                layout.first_id, layout.spacing_ratio, img_w as c_int, img_h as c_int, max_err_sq, max_drop, min_tags,
                                if predict_missing { ffi::AGX_FIT_PREDICT_MISSING } else { 0 }, h.as_mut_ptr(), err.as_mut_ptr(),
                                row_status.as_mut_ptr(), &mut n_inliers, &mut rms, pred.as_mut_ptr(), &mut n_pred, &mut status)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_board_fit_tail failed: {}", st);
    if status as c_int != ffi::AGX_FIT_OK && status as c_int != ffi::AGX_FIT_LOOSE {
        return Err(status);
    }
    Ok(BoardFit {
        status,
        h,
        rows: (0..tags.len()).map(|r| (row_status[r], err[r])).collect(),
        n_inliers: n_inliers as usize,
        rms,
        pred: pred[..n_pred as usize].iter()
            .map(|r| (r.id, [(r.xy[0], r.xy[1]), (r.xy[2], r.xy[3]), (r.xy[4], r.xy[5]), (r.xy[6], r.xy[7])])).collect(),
    })
}

/// `agx_camera`: the pinhole + radial-tangential model (OpenCV's; Kalibr's pinhole-radtan with `k3 = 0`).
#[derive(Clone, Copy, Debug, Default)]
pub struct Camera {
    pub fx: f64,
    pub fy: f64,
    pub cx: f64,
    pub cy: f64,
    pub k1: f64,
    pub k2: f64,
    pub p1: f64,
    pub p2: f64,
    pub k3: f64,
}

/// The lens model `board_pose_tail_m` reads a `Camera` under (`AGX_LENS_*`).
#[repr(i32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq, Default)]
pub enum LensModel {
    /// pinhole + radial-tangential: `Camera`'s fields as they are named
    #[default]
    Radtan = 0,
    /// pinhole-equidistant (Kalibr's pinhole-equi, OpenCV's fisheye): `Camera::equidistant`
    Equidistant = 1,
    /// double sphere (Usenko, Demmel, Cremers 2018; Kalibr's ds, Basalt's default): `Camera::double_sphere`
    DoubleSphere = 2,
}

impl Camera {
    /// The nine doubles of the pinhole-equidistant model, `fx, fy, cx, cy, k1, k2, k3, k4, 0`: `p1` holds `k3`, `p2` holds `k4`,
    /// `k3` is 0.  To be passed with `LensModel::Equidistant`.
    pub fn equidistant(fx: f64, fy: f64, cx: f64, cy: f64, k1: f64, k2: f64, k3: f64, k4: f64) -> Camera {
        Camera { fx, fy, cx, cy, k1, k2, p1: k3, p2: k4, k3: 0.0 }
    }

    /// The nine doubles of the double-sphere model, `fx, fy, cx, cy, xi, alpha, 0, 0, 0`: `k1` holds `xi` (in `(-1, 1]`), `k2` holds
    /// `alpha` (in `[0, 1]`).  To be passed with `LensModel::DoubleSphere`.  Points with `Z <= 0` inside the model's valid cone project.
    pub fn double_sphere(fx: f64, fy: f64, cx: f64, cy: f64, xi: f64, alpha: f64) -> Camera {
        Camera { fx, fy, cx, cy, k1: xi, k2: alpha, p1: 0.0, p2: 0.0, k3: 0.0 }
    }
}

/// What `board_pose_tail` found for one frame.
#[derive(Clone, Debug)]
pub struct BoardPose {
    /// `AGX_FIT_OK` or `AGX_FIT_LOOSE`
    pub status: u32,
    /// row major, board -> camera
    pub r: [f64; 9],
    /// in `tag_size`'s unit
    pub t: [f64; 3],
    /// the iterate of the last round that became the answer (0 = the pose the round started from)
    pub best_iter: u32,
    /// per row of the table: `AGX_FIT_ROW_*` and the squared residual in pixels (not written for an off-board row: NaN)
    pub rows: Vec<(u32, f32)>,
    pub n_inliers: usize,
    pub rms: f32,
    /// predicted tags in id order, through the lens model
    pub pred: Vec<(u32, [(f32, f32); 4])>,
}

/// The pose of the printed board in the camera frame (`Xc = R X + t`, board points in the plane Z = 0 centred on the board's
/// centre, times `tag_size`) under `camera` through every corner of a frame's tag table: a homography seed on undistorted corners,
/// `iterations` (0..=64) Gauss-Newton steps with the best iterate kept, `board_fit_tail`'s outlier rounds on the pose's residuals,
/// and the predicted corners of the layout's tags through the lens model.  The host form (no device is used).  `Err(status)`:
/// `AGX_FIT_FEW`, `AGX_FIT_SINGULAR` or `AGX_FIT_INPUT`.  Panics where the library refuses the arguments.
pub fn board_pose_tail(tags: &[(u32, [(f32, f32); 4])], layout: &BoardLayout, camera: &Camera, tag_size: f64, max_err_sq: f32, max_drop: u32,
                       min_tags: u32, iterations: u32, predict_missing: bool) -> Result<BoardPose, u32> {
    board_pose_tail_m(tags, layout, LensModel::Radtan, camera, tag_size, max_err_sq, max_drop, min_tags, iterations, predict_missing)
}

/// `board_pose_tail` under the lens model `model`: with `LensModel::Equidistant` and a `Camera::equidistant` the projection is
/// `theta = atan(r)`, `theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8)`, `(u, v) = (fx, fy) theta_d (x, y) / r + (cx, cy)`;
/// everything else is `board_pose_tail`'s.  `LensModel::Radtan` is that call, and its bytes.
pub fn board_pose_tail_m(tags: &[(u32, [(f32, f32); 4])], layout: &BoardLayout, model: LensModel, camera: &Camera, tag_size: f64, max_err_sq: f32,
                         max_drop: u32, min_tags: u32, iterations: u32, predict_missing: bool) -> Result<BoardPose, u32> {
    let table: Vec<ffi::agx_tag> = tags.iter().map(|t| ffi::agx_tag {
        id: t.0,
        xy: [t.1[0].0, t.1[0].1, t.1[1].0, t.1[1].1, t.1[2].0, t.1[2].1, t.1[3].0, t.1[3].1],
    }).collect();
    assert!(layout.cols > 0 && layout.rows > 0 && layout.cols as u64 * layout.rows as u64 <= 4096, "board_pose_tail: rows * cols in 1..=4096");
    let n_board = layout.cols as usize * layout.rows as usize;
    let cam = [camera.fx, camera.fy, camera.cx, camera.cy, camera.k1, camera.k2, camera.p1, camera.p2, camera.k3];
    let mut pose = [0f64; 12];
    let mut err = vec![f32::NAN; tags.len().max(1)];
    let mut row_status = vec![0u32; tags.len().max(1)];
    let mut pred = vec![ffi::agx_tag { id: 0, xy: [0.0; 8] }; n_board];
    let (mut n_inliers, mut n_pred, mut status, mut best_iter, mut rms) = (0u32, 0u32, 0u32, 0u32, 0f32);
    let st = unsafe {
        ffi::agx_board_pose_tail_m(table.as_ptr(), table.len() as u32, table.len() as u32, ffi::AGX_TAGS_OK as u32, layout.cols, layout.rows,
                                   layout.first_id, layout.spacing_ratio, tag_size, model as c_int, cam.as_ptr(), max_err_sq, max_drop, min_tags,
                                   iterations, if predict_missing { ffi::AGX_FIT_PREDICT_MISSING } else { 0 }, pose.as_mut_ptr(),
                                   err.as_mut_ptr(), row_status.as_mut_ptr(), &mut n_inliers, &mut rms, &mut best_iter, pred.as_mut_ptr(),
                                   &mut n_pred, &mut status)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_board_pose_tail_m failed: {}", st);
    if status as c_int != ffi::AGX_FIT_OK && status as c_int != ffi::AGX_FIT_LOOSE {
        return Err(status);
    }
    let (mut r, mut t) = ([0f64; 9], [0f64; 3]);
    r.copy_from_slice(&pose[..9]);
    t.copy_from_slice(&pose[9..]);
    Ok(BoardPose {
        status,
        r,
        t,
        best_iter,
        rows: (0..tags.len()).map(|k| (row_status[k], err[k])).collect(),
        n_inliers: n_inliers as usize,
        rms,
        pred: pred[..n_pred as usize].iter()
            .map(|q| (q.id, [(q.xy[0], q.xy[1]), (q.xy[2], q.xy[3]), (q.xy[4], q.xy[5]), (q.xy[6], q.xy[7])])).collect(),
    })
}

/// `agx_calib_report`: what `calibrate_tail` says about the call.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct CalibReport {
    /// `AGX_CALIB_OK`, `AGX_CALIB_FEW` or `AGX_CALIB_SINGULAR`
    pub status: u32,
    /// the iterate that became the answer (0 = the inputs)
    pub best_iter: u32,
    /// the last iterate that was evaluated
    pub iterations_run: u32,
    pub n_frames_used: u32,
    pub n_corners: u32,
    pub reserved: u32,
    /// the answer's RMS reprojection error in pixels
    pub rms: f64,
    /// the total squared residual of every iterate (NaN: not reached)
    pub cost: [f64; 65],
}

/// One frame of `calibrate_tail`: its tag table and what `board_pose_tail_m` found for it under the seed camera.
pub struct CalibFrame<'a> {
    pub tags: &'a [(u32, [(f32, f32); 4])],
    pub pose: &'a BoardPose,
}

/// The camera's nine doubles and every usable frame's pose from a batch of tag tables (`agx_calibrate_tail`, the host form: no
/// device is used): `iterations` (0..=64) damped Gauss-Newton steps over the camera's free doubles (`fixed_mask` bit i holds
/// double i) and all poses, the best iterate kept.  A frame is usable iff its pose's status is `AGX_FIT_OK` (`accept_loose`:
/// `AGX_FIT_LOOSE` too) and it has `min_tags` inlier rows.  -> the camera, the poses (12 doubles: R row major, then t; `None` for
/// a frame that was not usable) and the report; `Err(report)` under `AGX_CALIB_FEW` / `AGX_CALIB_SINGULAR`.  Panics where the
/// library refuses the arguments.
pub fn calibrate_tail(frames: &[CalibFrame], layout: &BoardLayout, model: LensModel, camera: &Camera, tag_size: f64, fixed_mask: u32, damping: f64,
                      iterations: u32, min_tags: u32, min_frames: u32, accept_loose: bool) -> Result<(Camera, Vec<Option<[f64; 12]>>, CalibReport), CalibReport> {
    let n = frames.len();
    let tpf = frames.iter().map(|f| f.tags.len()).max().unwrap_or(0).max(1);
    let mut table = vec![ffi::agx_tag { id: 0, xy: [0.0; 8] }; n * tpf];
    let mut row_status = vec![ffi::AGX_FIT_ROW_OFF_BOARD as u32; n * tpf];
    let (mut n_tags, mut fit_status, mut pose_in) = (vec![0u32; n], vec![0u32; n], vec![0f64; 12 * n]);
    for (f, fr) in frames.iter().enumerate() {
        for (k, t) in fr.tags.iter().enumerate() {
            table[f * tpf + k] = ffi::agx_tag { id: t.0, xy: [t.1[0].0, t.1[0].1, t.1[1].0, t.1[1].1, t.1[2].0, t.1[2].1, t.1[3].0, t.1[3].1] };
            row_status[f * tpf + k] = fr.pose.rows[k].0;
        }
        n_tags[f] = fr.tags.len() as u32;
        fit_status[f] = fr.pose.status;
        pose_in[12 * f..12 * f + 9].copy_from_slice(&fr.pose.r);
        pose_in[12 * f + 9..12 * f + 12].copy_from_slice(&fr.pose.t);
    }
    let cam = [camera.fx, camera.fy, camera.cx, camera.cy, camera.k1, camera.k2, camera.p1, camera.p2, camera.k3];
    let (mut cam_out, mut pose, mut cost, mut frame_n) = ([0f64; 9], vec![0f64; 12 * n], vec![0f32; n], vec![0u32; n]);
    let mut report = CalibReport { status: 0, best_iter: 0, iterations_run: 0, n_frames_used: 0, n_corners: 0, reserved: 0, rms: 0.0, cost: [0.0; 65] };
    let st = unsafe {
        ffi::agx_calibrate_tail(n as c_int, table.as_ptr(), tpf as u32, n_tags.as_ptr(), std::ptr::null(), layout.cols, layout.rows, layout.first_id,
                                layout.spacing_ratio, tag_size, model as c_int, cam.as_ptr(), fixed_mask, damping, iterations, min_tags, min_frames,
                                if accept_loose { ffi::AGX_CALIB_ACCEPT_LOOSE } else { 0 }, pose_in.as_ptr(), row_status.as_ptr(), fit_status.as_ptr(),
                                cam_out.as_mut_ptr(), pose.as_mut_ptr(), cost.as_mut_ptr(), frame_n.as_mut_ptr(),
                                &mut report as *mut CalibReport as *mut std::os::raw::c_void)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_calibrate_tail failed: {}", st);
    if report.status as c_int != ffi::AGX_CALIB_OK {
        return Err(report);
    }
    let c = Camera { fx: cam_out[0], fy: cam_out[1], cx: cam_out[2], cy: cam_out[3], k1: cam_out[4], k2: cam_out[5], p1: cam_out[6], p2: cam_out[7], k3: cam_out[8] };
    let poses = (0..n).map(|f| if frame_n[f] > 0 { let mut p = [0f64; 12]; p.copy_from_slice(&pose[12 * f..12 * f + 12]); Some(p) } else { None }).collect();
    Ok((c, poses, report))
}

/// The closed-form seed of a calibration (`agx_calibrate_seed_tail`, OpenCV's `initCameraMatrix2D`): a pinhole `Camera` with the
/// principal point at the image's centre and `fx`, `fy` from the homographies `h` (row major, board units -> pixels, `board_fit_tail`'s)
/// whose status word is `AGX_FIT_OK` or `AGX_FIT_LOOSE`.  `Err(AGX_CALIB_FEW | AGX_CALIB_SINGULAR)`.
pub fn calibrate_seed_tail(h: &[[f64; 9]], fit_status: &[u32], img_w: i32, img_h: i32) -> Result<Camera, u32> {
    assert!(!h.is_empty() && h.len() == fit_status.len(), "calibrate_seed_tail: one status word per homography");
    let (mut cam, mut status) = ([0f64; 9], 0u32);
    let st = unsafe { ffi::agx_calibrate_seed_tail(h.as_ptr() as *const f64, fit_status.as_ptr(), h.len() as u32, img_w, img_h, cam.as_mut_ptr(), &mut status) };
    assert_eq!(st, ffi::AGX_OK, "agx_calibrate_seed_tail failed: {}", st);
    if status as c_int != ffi::AGX_CALIB_OK {
        return Err(status);
    }
    Ok(Camera { fx: cam[0], fy: cam[1], cx: cam[2], cy: cam[3], k1: 0.0, k2: 0.0, p1: 0.0, p2: 0.0, k3: 0.0 })
}

/// `agx_rig_report`: what `rig_calibrate_tail` says about the call.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct RigReport {
    /// `AGX_RIG_OK`, `AGX_RIG_FEW` or `AGX_RIG_SINGULAR`
    pub status: u32,
    /// the iterate that became the answer (0 = the inputs)
    pub best_iter: u32,
    /// the last iterate that was evaluated
    pub iterations_run: u32,
    pub n_instants_used: u32,
    pub n_frames_used: u32,
    pub n_corners: u32,
    /// the cameras c >= 1 with a counted frame
    pub n_cams_free: u32,
    pub reserved: u32,
    /// the answer's RMS reprojection error in pixels
    pub rms: f64,
    /// the total squared residual of every iterate (NaN: not reached)
    pub cost: [f64; 65],
}

/// One camera of a rig for `rig_calibrate_tail`: its lens model and nine doubles (held), and its frames, one per instant.
pub struct RigCamera<'a> {
    pub model: LensModel,
    pub camera: Camera,
    pub frames: &'a [CalibFrame<'a>],
}

/// The extrinsics of a rig's cameras and the board's pose at every usable instant (`agx_rig_calibrate_tail`, the host form: no
/// device is used).  `cams`: 2..=8 cameras with one frame per instant each; `seed`: camera-from-rig per camera, 12 doubles (R row
/// major, then t; entry 0 is not read), `rig_seed_tail`'s.  An instant is usable iff `min_cams` of its frames are.  -> the
/// extrinsics (entry 0 the identity), the rig-from-board pose per instant (`None`: not usable) and the report; `Err(report)` under
/// `AGX_RIG_FEW` / `AGX_RIG_SINGULAR`.  Panics where the library refuses the arguments.
pub fn rig_calibrate_tail(cams: &[RigCamera], layout: &BoardLayout, tag_size: f64, seed: &[[f64; 12]], damping: f64, iterations: u32, min_tags: u32,
                          min_cams: u32, min_instants: u32, accept_loose: bool) -> Result<(Vec<[f64; 12]>, Vec<Option<[f64; 12]>>, RigReport), RigReport> {
    let (nc, ns) = (cams.len(), cams.first().map(|c| c.frames.len()).unwrap_or(0));
    assert!(seed.len() == nc && cams.iter().all(|c| c.frames.len() == ns), "rig_calibrate_tail: one seed per camera, one frame per camera and instant");
    let n = nc * ns;
    let tpf = cams.iter().flat_map(|c| c.frames.iter()).map(|f| f.tags.len()).max().unwrap_or(0).max(1);
    let mut table = vec![ffi::agx_tag { id: 0, xy: [0.0; 8] }; n * tpf];
    let mut row_status = vec![ffi::AGX_FIT_ROW_OFF_BOARD as u32; n * tpf];
    let (mut n_tags, mut fit_status, mut pose_in) = (vec![0u32; n], vec![0u32; n], vec![0f64; 12 * n]);
    let (mut models, mut cameras) = (vec![0 as c_int; nc], vec![0f64; 9 * nc]);
    for (c, cam) in cams.iter().enumerate() {
        models[c] = cam.model as c_int;
        let k = &cam.camera;
        cameras[9 * c..9 * c + 9].copy_from_slice(&[k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, k.k3]);
        for (s, fr) in cam.frames.iter().enumerate() {
            let f = c * ns + s;
            for (i, t) in fr.tags.iter().enumerate() {
                table[f * tpf + i] = ffi::agx_tag { id: t.0, xy: [t.1[0].0, t.1[0].1, t.1[1].0, t.1[1].1, t.1[2].0, t.1[2].1, t.1[3].0, t.1[3].1] };
                row_status[f * tpf + i] = fr.pose.rows[i].0;
            }
            n_tags[f] = fr.tags.len() as u32;
            fit_status[f] = fr.pose.status;
            pose_in[12 * f..12 * f + 9].copy_from_slice(&fr.pose.r);
            pose_in[12 * f + 9..12 * f + 12].copy_from_slice(&fr.pose.t);
        }
    }
    let ext_in: Vec<f64> = seed.iter().flat_map(|e| e.iter().copied()).collect();
    let (mut ext, mut rig_pose, mut cost, mut frame_n, mut cam_n) = (vec![0f64; 12 * nc], vec![0f64; 12 * ns], vec![0f32; n], vec![0u32; n], vec![0u32; nc]);
    let mut report = RigReport { status: 0, best_iter: 0, iterations_run: 0, n_instants_used: 0, n_frames_used: 0, n_corners: 0, n_cams_free: 0, reserved: 0,
                                 rms: 0.0, cost: [0.0; 65] };
    let st = unsafe {
        ffi::agx_rig_calibrate_tail(nc as c_int, ns as c_int, table.as_ptr(), tpf as u32, n_tags.as_ptr(), std::ptr::null(), layout.cols, layout.rows,
                                    layout.first_id, layout.spacing_ratio, tag_size, models.as_ptr(), cameras.as_ptr(), damping, iterations, min_tags,
                                    min_cams, min_instants, if accept_loose { ffi::AGX_CALIB_ACCEPT_LOOSE } else { 0 }, pose_in.as_ptr(),
                                    row_status.as_ptr(), fit_status.as_ptr(), ext_in.as_ptr(), ext.as_mut_ptr(), rig_pose.as_mut_ptr(), cost.as_mut_ptr(),
                                    frame_n.as_mut_ptr(), cam_n.as_mut_ptr(), &mut report as *mut RigReport as *mut std::os::raw::c_void)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_rig_calibrate_tail failed: {}", st);
    if report.status as c_int != ffi::AGX_RIG_OK {
        return Err(report);
    }
    let twelve = |v: &[f64], i: usize| { let mut p = [0f64; 12]; p.copy_from_slice(&v[12 * i..12 * i + 12]); p };
    let extrinsics = (0..nc).map(|c| twelve(&ext, c)).collect();
    let poses = (0..ns).map(|s| if (0..nc).any(|c| frame_n[c * ns + s] > 0) { Some(twelve(&rig_pose, s)) } else { None }).collect();
    Ok((extrinsics, poses, report))
}

/// The closed-form seed of a rig calibration (`agx_rig_seed_tail`): `pose[c][s]` (12 doubles) and `fit_status[c][s]` of
/// `board_pose_tail_m` per frame.  -> per camera its extrinsic, `None` for a camera that could not be attached.
pub fn rig_seed_tail(pose: &[Vec<[f64; 12]>], fit_status: &[Vec<u32>]) -> Vec<Option<[f64; 12]>> {
    let (nc, ns) = (pose.len(), pose.first().map(|p| p.len()).unwrap_or(0));
    assert!(fit_status.len() == nc && pose.iter().zip(fit_status).all(|(p, f)| p.len() == ns && f.len() == ns), "rig_seed_tail: one status word per pose");
    let flat: Vec<f64> = pose.iter().flat_map(|p| p.iter().flat_map(|e| e.iter().copied())).collect();
    let fst: Vec<u32> = fit_status.iter().flat_map(|f| f.iter().copied()).collect();
    let (mut ext, mut status) = (vec![0f64; 12 * nc], vec![0u32; nc]);
    let st = unsafe { ffi::agx_rig_seed_tail(nc as c_int, ns as c_int, flat.as_ptr(), fst.as_ptr(), std::ptr::null(), ext.as_mut_ptr(), status.as_mut_ptr()) };
    assert_eq!(st, ffi::AGX_OK, "agx_rig_seed_tail failed: {}", st);
    (0..nc).map(|c| if status[c] as c_int == ffi::AGX_RIG_CAM_ATTACHED { let mut p = [0f64; 12]; p.copy_from_slice(&ext[12 * c..12 * c + 12]); Some(p) } else { None }).collect()
}

/// The ideal pinhole a batch is rectified to, and the rotation from its frame to the camera's (`None`: the identity).
#[derive(Clone, Copy, Debug)]
pub struct Rectification {
    /// `fx', fy', cx', cy'`
    pub new_camera: [f64; 4],
    /// row major, rectified frame -> camera frame
    pub rotation: Option<[f64; 9]>,
}

fn camera_doubles(camera: &Camera) -> [f64; 9] {
    [camera.fx, camera.fy, camera.cx, camera.cy, camera.k1, camera.k2, camera.p1, camera.p2, camera.k3]
}

/// The rectification map of `camera` under `model`, the host form (no device is used): for every pixel of the `dst` = (w, h)
/// pinhole of `rect` the pixel of the `src` = (w, h) sensor image it comes from, `[mx, my]` in 1/32 px, row major, or
/// `[AGX_MAP_NONE; 2]` where the ray has no pixel there.  Panics where the library refuses the arguments.
pub fn rectify_map_tail(model: LensModel, camera: &Camera, rect: &Rectification, src: (u32, u32), dst: (u32, u32)) -> Vec<[i32; 2]> {
    let cam = camera_doubles(camera);
    let mut map = vec![[ffi::AGX_MAP_NONE; 2]; dst.0 as usize * dst.1 as usize];
    let st = unsafe {
        ffi::agx_rectify_map_tail(model as c_int, cam.as_ptr(), rect.new_camera.as_ptr(), rect.rotation.as_ref().map_or(std::ptr::null(), |r| r.as_ptr()),
                                  src.0 as c_int, src.1 as c_int, dst.0 as c_int, dst.1 as c_int, map.as_mut_ptr() as *mut c_int, 8 * dst.0 as usize)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_rectify_map_tail failed: {}", st);
    map
}

/// One tightly packed L8 frame of `src` = (w, h) through a map of `dst` = (w, h) entries, the host form: bilinear with 5-bit
/// weights in integers, `border` where the entry has no source pixel.  Panics where the library refuses the arguments.
pub fn remap_tail(frame: &[u8], src: (u32, u32), map: &[[i32; 2]], dst: (u32, u32), border: u8) -> Vec<u8> {
    assert_eq!(frame.len(), src.0 as usize * src.1 as usize, "remap_tail: frame is not w * h bytes");
    assert_eq!(map.len(), dst.0 as usize * dst.1 as usize, "remap_tail: map is not w * h entries");
    let mut out = vec![0u8; map.len()];
    let st = unsafe {
        ffi::agx_remap_tail(frame.as_ptr() as *const std::os::raw::c_void, 1, src.0 as c_int, src.1 as c_int, src.0 as usize, frame.len(), ffi::AGX_L8,
                            map.as_ptr() as *const c_int, 8 * dst.0 as usize, dst.0 as c_int, dst.1 as c_int,
                            out.as_mut_ptr() as *mut std::os::raw::c_void, dst.0 as usize, out.len(), border as u32)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_remap_tail failed: {}", st);
    out
}

/// One tightly packed L8 frame of `src` = (w, h) averaged down by `factor` in 2 .. 4, the host form: every output pixel the mean
/// of its `factor` x `factor` source pixels in integers, round half up; `(w / factor, h / factor)` pixels, row major.  The centre of
/// output pixel `(X, Y)` is the source position `(factor X + (factor - 1) / 2, factor Y + (factor - 1) / 2)`.  Panics where the
/// library refuses the arguments.
pub fn decimate_tail(frame: &[u8], src: (u32, u32), factor: u32) -> Vec<u8> {
    assert_eq!(frame.len(), src.0 as usize * src.1 as usize, "decimate_tail: frame is not w * h bytes");
    assert!((2..=4).contains(&factor) && src.0 >= factor && src.1 >= factor, "decimate_tail: factor must be in 2 .. 4 and no larger than a side");
    let (dw, dh) = ((src.0 / factor) as usize, (src.1 / factor) as usize);
    let mut out = vec![0u8; dw * dh];
    let st = unsafe {
        ffi::agx_decimate_tail(frame.as_ptr() as *const std::os::raw::c_void, 1, src.0 as c_int, src.1 as c_int, src.0 as usize, frame.len(), ffi::AGX_L8,
                               factor as c_int, out.as_mut_ptr() as *mut std::os::raw::c_void, dw, out.len())
    };
    assert_eq!(st, ffi::AGX_OK, "agx_decimate_tail failed: {}", st);
    out
}

/// Points of the rectified image to the sensor pixels they come from, the host form: the map's ray, rotation and projection in
/// binary64, rounded to `f32`; `(NaN, NaN)` where the ray has no projection.  Panics where the library refuses the arguments.
pub fn rectified_points_tail(model: LensModel, camera: &Camera, rect: &Rectification, points: &[(f32, f32)]) -> Vec<(f32, f32)> {
    let cam = camera_doubles(camera);
    let flat: Vec<f32> = points.iter().flat_map(|p| [p.0, p.1]).collect();
    let mut out = vec![0f32; flat.len()];
    let st = unsafe {
        ffi::agx_rectified_points_tail(model as c_int, cam.as_ptr(), rect.new_camera.as_ptr(),
                                       rect.rotation.as_ref().map_or(std::ptr::null(), |r| r.as_ptr()), flat.as_ptr() as *const std::os::raw::c_void, 8,
                                       points.len() as u32, out.as_mut_ptr() as *mut std::os::raw::c_void, 8)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_rectified_points_tail failed: {}", st);
    out.chunks(2).map(|c| (c[0], c[1])).collect()
}

/// What `render_boards_tail` drew: the L8 frame, row major, and the projected corners of every tag of the layout in id order.
#[derive(Clone, Debug)]
pub struct RenderedBoard {
    /// `AGX_RENDER_OK` or `AGX_RENDER_EMPTY`
    pub status: u32,
    pub frame: Vec<u8>,
    /// `(id, corners)`; `(NaN, NaN)` for a corner without a projection; empty unless `status` is `AGX_RENDER_OK`
    pub truth: Vec<(u32, [(f32, f32); 4])>,
}

/// The printed board of `layout` (tags of `family`) as `camera` under `model` sees it from the pose `r` (row major, board ->
/// camera), `t` in `tag_size`'s unit, the host form (no device is used): one tightly packed L8 frame of `size` = (w, h) drawn over
/// `background`, `supersample` x `supersample` samples a pixel, a white `page_margin` (tag sides) around the board.
/// `Err(AGX_RENDER_INPUT)`: a pose that is not finite or not a rotation.  Panics where the library refuses the arguments.
pub fn render_boards_tail(family: TagFamily, layout: &BoardLayout, model: LensModel, camera: &Camera, tag_size: f64, r: &[f64; 9], t: &[f64; 3],
                          size: (u32, u32), black: u8, white: u8, background: u8, page_margin: f32, supersample: u32) -> Result<RenderedBoard, u32> {
    let cam = camera_doubles(camera);
    let mut pose = [0f64; 12];
    pose[..9].copy_from_slice(r);
    pose[9..].copy_from_slice(t);
    let params = ffi::agx_render_params { black: black as u32, white: white as u32, background: background as u32, page_margin, supersample, flags: 0 };
    let n_board = layout.cols as usize * layout.rows as usize;
    let mut frame = vec![background; size.0 as usize * size.1 as usize];
    let mut truth = vec![ffi::agx_tag { id: 0, xy: [0.0; 8] }; n_board.max(1)];
    let (mut n_truth, mut status) = (0u32, 0u32);
    let st = unsafe {
        ffi::agx_render_boards_tail(size.0 as c_int, size.1 as c_int, size.0 as usize, ffi::AGX_L8, family as c_int, layout.cols, layout.rows,
                                    layout.first_id, layout.spacing_ratio, tag_size, model as c_int, cam.as_ptr(), pose.as_ptr(),
                                    &params as *const ffi::agx_render_params as *const std::os::raw::c_void,
                                    frame.as_mut_ptr() as *mut std::os::raw::c_void, truth.as_mut_ptr(), &mut n_truth, &mut status)
    };
    assert_eq!(st, ffi::AGX_OK, "agx_render_boards_tail failed: {}", st);
    if status as c_int == ffi::AGX_RENDER_INPUT {
        return Err(status);
    }
    Ok(RenderedBoard {
        status,
        frame,
        truth: truth[..n_truth as usize].iter()
            .map(|q| (q.id, [(q.xy[0], q.xy[1]), (q.xy[2], q.xy[3]), (q.xy[4], q.xy[5]), (q.xy[6], q.xy[7])])).collect(),
    })
}

fn last_error(det: *const ffi::agx_detector) -> String {
    unsafe {
        let p = ffi::agx_last_error(det);
        if p.is_null() { String::new() } else { std::ffi::CStr::from_ptr(p).to_string_lossy().into_owned() }
    }
}

//! hal_hip.rs — `impl Hal for HipHal`, `impl Buffer<T> for HipBuffer<T>` and `impl CircuitHal<HipHal> for HipCircuitHal` over
//! risc0-sys-hip (libzkhal_mi355x.so): the file a maintainer adds as `risc0-zkp/src/hal/hip.rs` behind `feature = "hip"`, next to
//! `hal/cuda.rs`.  It is what `default_prover().prove(env, elf)` (/root/reference/crates/host/src/lib.rs:137) ends up driving,
//! through `risc0_zkp::prove::Prover<'a, H: Hal>` inside the r0vm server.
//!
//! Written against the trait as RECALLED from risc0-zkp 3.0.2 `src/hal/mod.rs` (un-vendored: /root/reference/Cargo.lock:5393).
//! No Rust toolchain exists in the build image: this file has NOT been compiled.  What IS checked mechanically
//! (tests/test_rust_shim.py): every `zkh_*` call below names a function of the generated extern block with the right number of
//! arguments, and every method of the recalled `Hal` / `Buffer` / `CircuitHal` traits has a body here — none is elided.
//!
//! Conventions: `Elem` = 1 word, `ExtElem` = 4 words, `Digest` = 8 words, all raw Montgomery `u32`s exactly as upstream stores
//! them (`bytemuck::cast_slice` is enough in both directions).  One `HipHal` = one GPU + one in-order HIP stream, driven by the
//! single prover thread (upstream HALs are `!Sync` in practice too); `Buffer` handles are reference counted inside the library.

use std::cell::RefCell;
use std::ffi::CString;
use std::fmt::Debug;
use std::marker::PhantomData;
use std::rc::Rc;

use bytemuck::Pod;
use risc0_core::field::baby_bear::{BabyBear, BabyBearElem, BabyBearExtElem};
use risc0_sys_hip as sys;
use risc0_sys_hip::{ffi_wrap, ZkhBuf, ZkhCircuit, ZkhCtx};

use crate::core::digest::Digest;
use crate::core::hash::{poseidon2::Poseidon2HashSuite, HashSuite};
use crate::hal::{Buffer, CircuitHal, Hal};
use crate::INV_RATE;

/// Words per element of the three payload types (`u32` itself: 1).
fn words_of<T>() -> usize {
    std::mem::size_of::<T>() / 4
}

fn ffi<F: FnOnce() -> *const std::os::raw::c_char>(f: F) {
    // upstream's CUDA HAL panics on a failed kernel too (`ffi_wrap(..).unwrap()`): a HAL op has no error channel in the trait
    ffi_wrap(f).unwrap()
}

struct CtxHandle(*mut ZkhCtx);
impl Drop for CtxHandle {
    fn drop(&mut self) {
        unsafe { sys::zkh_ctx_destroy(self.0) }
    }
}

/// `impl Hal`: one MI355X.
pub struct HipHal {
    ctx: Rc<CtxHandle>,
    suite: HashSuite<BabyBear>,
}

/// `impl Buffer<T>`: a reference-counted view {allocation, offset, length} inside the library.
pub struct HipBuffer<T> {
    raw: *mut ZkhBuf,
    ctx: Rc<CtxHandle>,
    name: &'static str,
    _t: PhantomData<T>,
}

impl<T> Clone for HipBuffer<T> {
    fn clone(&self) -> Self {
        unsafe { sys::zkh_retain(self.raw) };
        HipBuffer { raw: self.raw, ctx: self.ctx.clone(), name: self.name, _t: PhantomData }
    }
}

impl<T> Drop for HipBuffer<T> {
    fn drop(&mut self) {
        unsafe { sys::zkh_release(self.raw) }
    }
}

impl<T: Pod> HipBuffer<T> {
    fn read_words(&self, off_items: usize, n_items: usize) -> Vec<u32> {
        let w = words_of::<T>();
        let mut host = vec![0u32; n_items * w];
        ffi(|| unsafe { sys::zkh_read(self.ctx.0, self.raw, host.as_mut_ptr(), off_items * w, n_items * w) });
        host
    }
}

impl<T: Pod + Clone> Buffer<T> for HipBuffer<T> {
    fn name(&self) -> &'static str {
        self.name
    }

    fn size(&self) -> usize {
        unsafe { sys::zkh_size(self.raw) } / words_of::<T>()
    }

    fn slice(&self, offset: usize, size: usize) -> Self {
        let w = words_of::<T>();
        let mut out: *mut ZkhBuf = std::ptr::null_mut();
        ffi(|| unsafe { sys::zkh_slice(self.raw, offset * w, size * w, &mut out) });
        HipBuffer { raw: out, ctx: self.ctx.clone(), name: self.name, _t: PhantomData }
    }

    fn get_at(&self, idx: usize) -> T {
        let words = self.read_words(idx, 1);
        bytemuck::cast_slice::<u32, T>(&words)[0]
    }

    fn view<F: FnOnce(&[T])>(&self, f: F) {
        let words = self.read_words(0, self.size()); // synchronises the stream, then D2H
        f(bytemuck::cast_slice::<u32, T>(&words))
    }

    fn view_mut<F: FnOnce(&mut [T])>(&self, f: F) {
        let mut words = self.read_words(0, self.size());
        f(bytemuck::cast_slice_mut::<u32, T>(&mut words));
        ffi(|| unsafe { sys::zkh_write(self.ctx.0, self.raw, words.as_ptr(), 0, words.len()) });
    }

    fn to_vec(&self) -> Vec<T> {
        let words = self.read_words(0, self.size());
        bytemuck::cast_slice::<u32, T>(&words).to_vec()
    }
}

impl HipHal {
    /// `CudaHal::new` analogue: binds `device_ordinal` (one r0vm worker per GPU: HIP_VISIBLE_DEVICES=k, ordinal 0).
    pub fn new(device_ordinal: i32) -> Self {
        let suite_name = CString::new("poseidon2").unwrap();
        let mut ctx: *mut ZkhCtx = std::ptr::null_mut();
        ffi(|| unsafe { sys::zkh_ctx_create(device_ordinal, suite_name.as_ptr(), &mut ctx) });
        // bind the prover thread (and the pinned blocks it allocates) next to the GPU's root port; a no-op where the host reports no node
        ffi(|| unsafe { sys::zkh_bind_thread_to_device(device_ordinal, 0, 1, std::ptr::null_mut(), std::ptr::null_mut()) });
        HipHal { ctx: Rc::new(CtxHandle(ctx)), suite: Poseidon2HashSuite::new_suite() }
    }

    fn alloc<T: Pod>(&self, name: &'static str, items: usize, zero: bool) -> HipBuffer<T> {
        let cname = CString::new(name).unwrap();
        let mut out: *mut ZkhBuf = std::ptr::null_mut();
        ffi(|| unsafe { sys::zkh_alloc(self.ctx.0, cname.as_ptr(), items * words_of::<T>(), zero as i32, &mut out) });
        HipBuffer { raw: out, ctx: self.ctx.clone(), name, _t: PhantomData }
    }

    fn copy_from<T: Pod>(&self, name: &'static str, slice: &[T]) -> HipBuffer<T> {
        let cname = CString::new(name).unwrap();
        let words: &[u32] = bytemuck::cast_slice(slice);
        let mut out: *mut ZkhBuf = std::ptr::null_mut();
        ffi(|| unsafe { sys::zkh_copy_from(self.ctx.0, cname.as_ptr(), words.as_ptr(), words.len(), &mut out) });
        HipBuffer { raw: out, ctx: self.ctx.clone(), name, _t: PhantomData }
    }

    fn ext_words(e: &BabyBearExtElem) -> *const u32 {
        e as *const BabyBearExtElem as *const u32 // 4 Montgomery words, the layout `ExtElem::to_u32_words` has
    }
}

impl Hal for HipHal {
    type Field = BabyBear;
    type Elem = BabyBearElem;
    type ExtElem = BabyBearExtElem;
    type Buffer<T: Clone + Debug + PartialEq> = HipBuffer<T>;

    fn has_unified_memory(&self) -> bool {
        false
    }

    fn get_hash_suite(&self) -> &HashSuite<Self::Field> {
        &self.suite // the Fiat-Shamir sponge / WriteIOP stay upstream's host code
    }

    fn alloc_digest(&self, name: &'static str, size: usize) -> Self::Buffer<Digest> {
        self.alloc(name, size, false)
    }

    fn alloc_elem(&self, name: &'static str, size: usize) -> Self::Buffer<Self::Elem> {
        self.alloc(name, size, false)
    }

    fn alloc_elem_init(&self, name: &'static str, size: usize, value: Self::Elem) -> Self::Buffer<Self::Elem> {
        self.copy_from(name, &vec![value; size])
    }

    fn alloc_extelem(&self, name: &'static str, size: usize) -> Self::Buffer<Self::ExtElem> {
        self.alloc(name, size, false)
    }

    fn alloc_extelem_zeroed(&self, name: &'static str, size: usize) -> Self::Buffer<Self::ExtElem> {
        self.alloc(name, size, true) // Montgomery zero is the all-zero word
    }

    fn alloc_u32(&self, name: &'static str, size: usize) -> Self::Buffer<u32> {
        self.alloc(name, size, false)
    }

    fn copy_from_digest(&self, name: &'static str, slice: &[Digest]) -> Self::Buffer<Digest> {
        self.copy_from(name, slice)
    }

    fn copy_from_elem(&self, name: &'static str, slice: &[Self::Elem]) -> Self::Buffer<Self::Elem> {
        self.copy_from(name, slice)
    }

    fn copy_from_extelem(&self, name: &'static str, slice: &[Self::ExtElem]) -> Self::Buffer<Self::ExtElem> {
        self.copy_from(name, slice)
    }

    fn copy_from_u32(&self, name: &'static str, slice: &[u32]) -> Self::Buffer<u32> {
        self.copy_from(name, slice)
    }

    fn batch_expand_into_evaluate_ntt(&self, output: &Self::Buffer<Self::Elem>, input: &Self::Buffer<Self::Elem>, count: usize, expand_bits: usize) {
        ffi(|| unsafe { sys::zkh_batch_expand_into_evaluate_ntt(self.ctx.0, output.raw, input.raw, count, expand_bits) });
    }

    fn batch_interpolate_ntt(&self, io: &Self::Buffer<Self::Elem>, count: usize) {
        ffi(|| unsafe { sys::zkh_batch_interpolate_ntt(self.ctx.0, io.raw, count) });
    }

    fn batch_bit_reverse(&self, io: &Self::Buffer<Self::Elem>, count: usize) {
        ffi(|| unsafe { sys::zkh_batch_bit_reverse(self.ctx.0, io.raw, count) });
    }

    fn batch_evaluate_any(&self, coeffs: &Self::Buffer<Self::Elem>, poly_count: usize, which: &Self::Buffer<u32>, xs: &Self::Buffer<Self::ExtElem>, out: &Self::Buffer<Self::ExtElem>) {
        ffi(|| unsafe { sys::zkh_batch_evaluate_any(self.ctx.0, coeffs.raw, poly_count, which.raw, xs.raw, out.raw) });
    }

    fn zk_shift(&self, io: &Self::Buffer<Self::Elem>, count: usize) {
        ffi(|| unsafe { sys::zkh_zk_shift(self.ctx.0, io.raw, count) });
    }

    fn mix_poly_coeffs(&self, output: &Self::Buffer<Self::ExtElem>, mix_start: &Self::ExtElem, mix: &Self::ExtElem, input: &Self::Buffer<Self::Elem>, combos: &Self::Buffer<u32>, input_size: usize, count: usize) {
        ffi(|| unsafe { sys::zkh_mix_poly_coeffs(self.ctx.0, output.raw, Self::ext_words(mix_start), Self::ext_words(mix), input.raw, combos.raw, input_size, count) });
    }

    fn eltwise_add_elem(&self, output: &Self::Buffer<Self::Elem>, input1: &Self::Buffer<Self::Elem>, input2: &Self::Buffer<Self::Elem>) {
        ffi(|| unsafe { sys::zkh_eltwise_add_elem(self.ctx.0, output.raw, input1.raw, input2.raw) });
    }

    fn eltwise_sum_extelem(&self, output: &Self::Buffer<Self::Elem>, input: &Self::Buffer<Self::ExtElem>) {
        ffi(|| unsafe { sys::zkh_eltwise_sum_extelem(self.ctx.0, output.raw, input.raw) });
    }

    fn eltwise_copy_elem(&self, output: &Self::Buffer<Self::Elem>, input: &Self::Buffer<Self::Elem>) {
        ffi(|| unsafe { sys::zkh_eltwise_copy_elem(self.ctx.0, output.raw, input.raw) });
    }

    fn eltwise_zeroize_elem(&self, elems: &Self::Buffer<Self::Elem>) {
        ffi(|| unsafe { sys::zkh_eltwise_zeroize_elem(self.ctx.0, elems.raw) });
    }

    fn fri_fold(&self, output: &Self::Buffer<Self::Elem>, input: &Self::Buffer<Self::Elem>, mix: &Self::ExtElem) {
        ffi(|| unsafe { sys::zkh_fri_fold(self.ctx.0, output.raw, input.raw, Self::ext_words(mix)) });
    }

    fn hash_rows(&self, output: &Self::Buffer<Digest>, matrix: &Self::Buffer<Self::Elem>) {
        ffi(|| unsafe { sys::zkh_hash_rows(self.ctx.0, output.raw, matrix.raw) });
    }

    fn hash_fold(&self, io: &Self::Buffer<Digest>, input_size: usize, output_size: usize) {
        ffi(|| unsafe { sys::zkh_hash_fold(self.ctx.0, io.raw, input_size, output_size) });
    }

    fn gather_sample(&self, dst: &Self::Buffer<Self::Elem>, src: &Self::Buffer<Self::Elem>, idx: usize, size: usize, stride: usize) {
        ffi(|| unsafe { sys::zkh_gather_sample(self.ctx.0, dst.raw, src.raw, idx, size, stride) });
    }

    fn scatter(&self, into: &Self::Buffer<Self::Elem>, index: &[u32], offsets: &[u32], values: &[Self::Elem]) {
        let vals: &[u32] = bytemuck::cast_slice(values);
        ffi(|| unsafe { sys::zkh_scatter(self.ctx.0, into.raw, index.as_ptr(), offsets.as_ptr(), vals.as_ptr(), index.len(), vals.len()) });
    }

    fn prefix_products(&self, io: &Self::Buffer<Self::ExtElem>) {
        ffi(|| unsafe { sys::zkh_prefix_products(self.ctx.0, io.raw) });
    }

    fn combos_prepare(&self, combos: &Self::Buffer<Self::ExtElem>, coeff_u: &Self::Buffer<Self::ExtElem>, combo_count: usize, cycles: usize, reg_sizes: &Self::Buffer<u32>, reg_combo_ids: &Self::Buffer<u32>, mix: &Self::ExtElem) {
        ffi(|| unsafe { sys::zkh_combos_prepare_regs(self.ctx.0, combos.raw, coeff_u.raw, combo_count, cycles, reg_sizes.size(), reg_sizes.raw, reg_combo_ids.raw, Self::ext_words(mix)) });
    }

    fn combos_divide(&self, combos: &Self::Buffer<Self::ExtElem>, chunks: Vec<(usize, Vec<Self::ExtElem>)>, cycles: usize) {
        // upstream: for every (combo, points) divide combo `combo` by (x - p) for each p in turn; the remainders must vanish
        for (combo, points) in chunks {
            let pts: &[u32] = bytemuck::cast_slice(&points);
            let rem = self.alloc::<Self::ExtElem>("combos_rem", points.len(), true);
            ffi(|| unsafe { sys::zkh_combos_divide(self.ctx.0, combos.raw, combo, cycles, pts.as_ptr(), points.len(), rem.raw) });
            rem.view(|r| debug_assert!(r.iter().all(|x| *x == Self::ExtElem::ZERO), "combos_divide: nonzero remainder"));
        }
    }
}

/// `impl CircuitHal<HipHal>`: a circuit is DATA here — the TapSet + PolyExtStep list of the upstream circuit crate
/// (`src/zirgen/{taps.rs, poly_ext.rs}`) serialised into the desc blob `tools/import_upstream_circuit.py` writes, loaded once;
/// its straight-line `eval_check` kernels are attached as code objects (`python -m zeth_amd.circuits.jit circuit.desc outdir/`).
pub struct HipCircuitHal {
    hal: Rc<HipHal>,
    circuit: *mut ZkhCircuit,
    kernels: RefCell<usize>,
}

impl HipCircuitHal {
    pub fn new(hal: Rc<HipHal>, desc: &[u32]) -> Self {
        let mut circuit: *mut ZkhCircuit = std::ptr::null_mut();
        ffi(|| unsafe { sys::zkh_circuit_load(hal.ctx.0, desc.as_ptr(), desc.len(), &mut circuit) });
        HipCircuitHal { hal, circuit, kernels: RefCell::new(0) }
    }

    /// One generated kernel (`.hsaco` image + its entry point) of `n_parts`; without any the on-device step interpreter runs.
    pub fn attach_code_object(&self, image: &[u8], kernel_name: &str, part: usize, n_parts: usize) {
        let name = CString::new(kernel_name).unwrap();
        ffi(|| unsafe { sys::zkh_circuit_attach_code_object_part(self.circuit, image.as_ptr() as *const _, image.len(), name.as_ptr(), part, n_parts) });
        *self.kernels.borrow_mut() = unsafe { sys::zkh_circuit_compiled_parts(self.circuit) };
    }

    /// The circuit's lookup / permutation arguments as a ZKA1 blob (`zeth_amd/circuits/logup.py`): `accumulate` then builds the accum
    /// group on the device (`zkh_accumulate`).  Validated against the circuit; an empty blob removes them.
    pub fn set_arguments(&self, blob: &[u32]) {
        ffi(|| unsafe { sys::zkh_circuit_set_arguments(self.circuit, blob.as_ptr(), blob.len()) });
    }

    pub fn has_arguments(&self) -> bool {
        unsafe { sys::zkh_circuit_has_arguments(self.circuit) != 0 }
    }

    /// The arguments (a ZKA1 version-2 blob) mark a lookup table's multiplicity as derived by the library.
    pub fn derives_multiplicities(&self) -> bool {
        unsafe { sys::zkh_circuit_derives_multiplicities(self.circuit) != 0 }
    }

    /// Fill everything the arguments derive into `data` from the raw code (ctrl) and data traces (`zkh_derive_all`), after the data
    /// upload and before the data group is committed (`prove_begin`): the stages below in the one order in which they are sound
    /// (sorted, columns, links, multiplicities), each only if the circuit has it; nothing to derive is a no-op.  Panics on the first
    /// stage that refuses the witness; the stages before it have written their columns.
    pub fn derive_all(&self, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_derive_all(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, ctrl.raw, data.raw) });
    }

    /// Fill the derived multiplicity columns of `data` on the active rows from the raw code (ctrl) and data traces
    /// (`zkh_derive_multiplicities`).  Panics on a refused witness (a table selector other than 0 / 1, a lookup without a table
    /// entry), which leaves `data` unchanged, like every failed HAL op.
    pub fn derive_multiplicities(&self, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_derive_multiplicities(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, ctrl.raw, data.raw) });
    }

    /// The arguments (a ZKA1 version-3 blob) mark a term as a sorted copy derived by the library.
    pub fn derives_sorted(&self) -> bool {
        unsafe { sys::zkh_circuit_derives_sorted(self.circuit) != 0 }
    }

    /// Fill the tuple columns of the derived sorted copies of `data` on the active rows from the raw code (ctrl) and data traces
    /// (`zkh_derive_sorted`): each source tuple's selected rows, stably sorted by its key columns.  Panics on a refused witness (a
    /// selector other than 0 / 1), which leaves `data` unchanged, like every failed HAL op.
    pub fn derive_sorted(&self, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_derive_sorted(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, ctrl.raw, data.raw) });
    }

    /// The arguments (a ZKA1 version-4 blob) hold derived-column records (LIMBS / ORDER) that the library fills.
    pub fn derives_columns(&self) -> bool {
        unsafe { sys::zkh_circuit_derives_columns(self.circuit) != 0 }
    }

    /// Fill the destination columns of the derived-column records of `data` on the active rows (`zkh_derive_columns`): the limbs of a
    /// word, or the flag and difference limbs that witness the order of sorted keys.  Panics on a refused witness (a value that does
    /// not fit its limbs, keys that are not in order), which leaves `data` unchanged.
    pub fn derive_columns(&self, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_derive_columns(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, ctrl.raw, data.raw) });
    }

    /// The arguments (a ZKA1 version-5 blob) hold LINK records that the library fills.
    pub fn derives_links(&self) -> bool {
        unsafe { sys::zkh_circuit_derives_links(self.circuit) != 0 }
    }

    /// The LINK records with READS (a ZKA1 version-6 blob): `derive_links` then refuses a load that does not return the last store, or
    /// 0 from an address never accessed, as well.
    pub fn links_check_reads(&self) -> usize {
        unsafe { sys::zkh_circuit_links_check_reads(self.circuit) as usize }
    }

    /// Fill the destination columns of the LINK records of `data` on the active rows (`zkh_derive_links`): every memory access gets
    /// the previous access to its own address (linked, last, the carried values, the limbs of the clock difference).  Panics on a
    /// refused witness (a selector other than 0 / 1, a clock that does not increase, a difference that does not fit its limbs), which
    /// leaves `data` unchanged.  LINK records that join a head (ZKA1 version 9) are the ports of one memory: the previous access is
    /// then the one before it in (row, port) order, in whichever port.
    pub fn derive_links(&self, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_derive_links(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, ctrl.raw, data.raw) });
    }

    /// The arguments (a ZKA1 version-7 blob) hold a PAGES record: the memory of its LINK record starts from an image
    /// (`derive_links_paged`, `derive_all_paged`) and `page_out` writes it back; `derive_links` and `derive_all` refuse such a circuit.
    pub fn pages(&self) -> bool {
        unsafe { sys::zkh_circuit_pages(self.circuit) != 0 }
    }

    /// V, the value words per address of the paged memory (`zkh_circuit_page_words`): 0 without a PAGES record, else 1 or (ZKA1
    /// version 10: the paged LINK carries two values) 2.  The image is then V W words, word j of address a at V a + j.
    pub fn page_words(&self) -> usize {
        unsafe { sys::zkh_circuit_page_words(self.circuit) as usize }
    }

    /// F, the flat-address destinations of the PAGES record (`zkh_circuit_page_flats`): 2 when the links stage writes
    /// `p_flat_j = 2 a + j` beside a wide page table (ZKA1 version 11), which the tie of a wide memory needs; else 0.
    pub fn page_flats(&self) -> usize {
        unsafe { sys::zkh_circuit_page_flats(self.circuit) as usize }
    }

    /// `derive_links` from a memory image of raw Montgomery words (`zkh_derive_links_paged`): an unlinked access of the paged LINK
    /// record takes `image[address]` as its previous access (at clock 0), and the PAGES record's page table is written.  Panics on a
    /// refused witness as `derive_links` does, and on an address outside the image, a clock 0 or an unlinked load that does not return
    /// the image's word; `data` is then unchanged.  Without a PAGES record the image is ignored.
    pub fn derive_links_paged(&self, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, image: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_derive_links_paged(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, ctrl.raw, data.raw, image.raw) });
    }

    /// `derive_all` with the memory image that the links stage of a paging circuit reads (`zkh_derive_all_paged`).
    pub fn derive_all_paged(&self, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, image: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_derive_all_paged(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, ctrl.raw, data.raw, image.raw) });
    }

    /// `derive_links_paged` from the page table of a ZKU1 proof in the image's place (`zkh_derive_links_paged_table`): the words of
    /// `table` from `table_at` on are `rows` rows (address, in, out) over an image of `image_words` words (for a proof `table_at = 5 + h`),
    /// and row i's `in` stands for `image[a_i]`.  The result is `derive_links_paged`'s on the image the table was made from, cell for
    /// cell as residues.  Panics as `derive_links_paged` does, and when the table's rows are not the trace's pages; `data` is then unchanged.
    pub fn derive_links_paged_table(&self, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, table: &HipBuffer<u32>, table_at: usize, rows: usize,
                                    image_words: usize, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_derive_links_paged_table(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, ctrl.raw, data.raw, table.raw, table_at, rows, image_words) });
    }

    /// `derive_all_paged` with that page table where the links stage gets the image (`zkh_derive_all_paged_table`).
    pub fn derive_all_paged_table(&self, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, table: &HipBuffer<u32>, table_at: usize, rows: usize,
                                  image_words: usize, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_derive_all_paged_table(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, ctrl.raw, data.raw, table.raw, table_at, rows, image_words) });
    }

    /// Write the page table of `data` back into `image` (`zkh_page_out`): `image[p_addr] = p_out` on every active row with `p_on` = 1.
    /// A call of its own, after the seal, so that a refused or aborted seal never touches the image.  Panics, with the image unchanged,
    /// on a `p_on` other than 0 / 1, an address outside the image, or page addresses that do not strictly increase over a prefix of rows.
    pub fn page_out(&self, data: &HipBuffer<BabyBearElem>, image: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_page_out(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, data.raw, image.raw) });
    }

    /// The words of the committed tree of an image of `image_words` words (`zkh_image_tree_words`): 16 L, L the smallest power of two
    /// >= ceil(W / 8); 0 for an empty image.
    pub fn image_tree_words(image_words: usize) -> usize {
        unsafe { sys::zkh_image_tree_words(image_words) }
    }

    /// Commit to a memory image (`zkh_image_commit`): `nodes` (exactly `image_tree_words` words) becomes 2 L digests in heap order, the
    /// leaves the image's residues mod P eight at a time and zero-padded, every node above `hash_pair` of its two children, the root
    /// digest 1.  Panics on an empty image or a `nodes` of another size.
    pub fn image_commit(&self, image: &HipBuffer<BabyBearElem>, nodes: &HipBuffer<BabyBearElem>) {
        ffi(|| unsafe { sys::zkh_image_commit(self.hal.ctx.0, image.raw, nodes.raw) });
    }

    /// `page_out`, and `nodes` (the committed tree of `image` before the call) brought up to the new image by hashing only the paths of
    /// the paged words again (`zkh_page_out_tree`): afterwards `nodes` is word for word what `image_commit` writes for the new image.
    /// Panics as `page_out` does, and on a `nodes` of the wrong size; image and nodes are then unchanged.
    pub fn page_out_tree(&self, data: &HipBuffer<BabyBearElem>, image: &HipBuffer<BabyBearElem>, nodes: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_page_out_tree(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, data.raw, image.raw, nodes.raw) });
    }

    /// The bound on the words of a ZKU1 proof of `pages` pages over an image of `image_words` words (`zkh_image_proof_words`).
    pub fn image_proof_words(image_words: usize, pages: usize) -> usize {
        unsafe { sys::zkh_image_proof_words(image_words, pages) }
    }

    /// The ZKU1 proof of the page-out of `data`'s page table (`zkh_page_out_proof`): the table's rows, the old leaves they touch and the
    /// clean sibling digests of every layer, from which the root of `nodes` and the root after the page-out both follow.  Only reads
    /// `data`, `image` and `nodes` (the committed tree of `image` as it is): call it before `page_out_tree`.  `proof` holds at least
    /// `image_proof_words(W, pages)` words; the proof's own length follows from its header.  Panics as `page_out` does, when a `p_in` is
    /// not the word the tree holds, and on a `nodes` or `proof` of the wrong size.
    pub fn page_out_proof(&self, data: &HipBuffer<BabyBearElem>, image: &HipBuffer<BabyBearElem>, nodes: &HipBuffer<BabyBearElem>, proof: &HipBuffer<u32>,
                          steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_page_out_proof(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, data.raw, image.raw, nodes.raw, proof.raw) });
    }

    /// Walk a ZKU1 proof from `root_before` to the root after the page-out (`zkh_image_proof_verify`): host only, no GPU.  Panics with
    /// one message per cause when the proof is refused.
    pub fn image_proof_verify(proof: &[u32], root_before: &[u32; 8]) -> [u32; 8] {
        let mut after = [0u32; 8];
        ffi(|| unsafe { sys::zkh_image_proof_verify(proof.as_ptr(), proof.len(), root_before.as_ptr(), after.as_mut_ptr()) });
        after
    }

    /// The same walk on the device (`zkh_image_proof_walk`): the first `words` words of the device buffer `proof` are the ZKU1 proof
    /// (the buffer `page_out_proof` wrote goes in as it is, with the proof's own length); the buffer is only read.  The same root, and
    /// the same message per cause, as `image_proof_verify` gives on the host.
    pub fn image_proof_walk(&self, proof: &HipBuffer<u32>, words: usize, root_before: &[u32; 8]) -> [u32; 8] {
        let mut after = [0u32; 8];
        ffi(|| unsafe { sys::zkh_image_proof_walk(self.hal.ctx.0, proof.raw, words, root_before.as_ptr(), after.as_mut_ptr()) });
        after
    }

    /// The bound on the words of the dirty-node table of a page-out of `pages` rows over an image of `image_words` words
    /// (`zkh_image_dirty_words`): 4 + h + 33 sum_k min(pages, L >> k).
    pub fn image_dirty_words(image_words: usize, pages: usize) -> usize {
        unsafe { sys::zkh_image_dirty_words(image_words, pages) }
    }

    /// `image_proof_walk` that keeps what it recomputes (`zkh_image_proof_nodes`): on success `dirty` (at least `image_dirty_words(W, D)`
    /// words) starts with the dirty-node table of the page-out, what `page_tree_witgen_nodes` reads in place of the two trees.  The
    /// walk's root and the walk's message per cause; `dirty` is written only on success; an empty table (D = 0) panics: it is sealed
    /// from the tree.
    pub fn image_proof_nodes(&self, proof: &HipBuffer<u32>, words: usize, root_before: &[u32; 8], dirty: &HipBuffer<u32>) -> [u32; 8] {
        let mut after = [0u32; 8];
        ffi(|| unsafe { sys::zkh_image_proof_nodes(self.hal.ctx.0, proof.raw, words, root_before.as_ptr(), after.as_mut_ptr(), dirty.raw) });
        after
    }

    /// The code group of P2-PAGE, the circuit that seals a page-out from root to root (`zkh_page_circuit_code`): a function of the trace's
    /// size and of the tree height of an image of `image_words` words.  `self` holds the P2-PAGE description.  Panics on a circuit of
    /// another shape, on `image_words <= 8`, and on a trace without room for one path.
    pub fn page_circuit_code(&self, image_words: usize, code: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_page_circuit_code(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, image_words, code.raw) });
    }

    /// The data group of P2-PAGE for the page-out a ZKU1 proof describes (`zkh_page_circuit_witgen`) and the `out` globals, root_before
    /// then root_after.  Only the header and the table of the first `words` words of `proof` are read; `nodes_before` / `nodes_after`
    /// are the committed tree before and after `page_out_tree`; `code` is `page_circuit_code` of the same image size.  `noise_key`:
    /// the 256-bit key of the blinding rows, `None` for fresh OS randomness.  Panics with one message per cause: a proof header that
    /// does not fit, more updates than the trace has paths, trees of another size, a code group of another tree height, an address
    /// outside the image or out of order.
    pub fn page_circuit_witgen(&self, code: &HipBuffer<BabyBearElem>, proof: &HipBuffer<u32>, words: usize, nodes_before: &HipBuffer<BabyBearElem>,
                               nodes_after: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, steps: usize, noise_key: Option<&[u32; 8]>) -> [u32; 16] {
        let po2 = steps.trailing_zeros() as usize;
        let mut roots = [0u32; 16];
        ffi(|| unsafe { sys::zkh_page_circuit_witgen(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, code.raw, proof.raw, words, nodes_before.raw, nodes_after.raw,
                                                     data.raw, roots.as_mut_ptr(), noise_key.map_or(std::ptr::null(), |k| k.as_ptr())) });
        roots
    }

    /// N, the path slots of a P2-PAGE trace of `steps` rows over an image of `image_words` words (`zkh_page_circuit_slots`): host only, no
    /// GPU; 0 where `page_circuit_code` refuses the shape.  A table of D rows is sealed as the parts that start at 0, N, 2 N, ... below
    /// D (D = 0: one part at 0).
    pub fn page_circuit_slots(image_words: usize, steps: usize) -> usize {
        unsafe { sys::zkh_page_circuit_slots(steps.trailing_zeros() as usize, sys::ZK_CYCLES, image_words) }
    }

    /// The data group of P2-PAGE for ONE PART of a page-out (`zkh_page_circuit_witgen_part`): the updates `first .. first + min(N, D -
    /// first)` of the proof's table, and the `out` globals, the root before update `first` then the root after the part's last update.
    /// The other operands are `page_circuit_witgen`'s; both trees are the whole page-out's for every part, so the parts can be generated
    /// in any order.  Part p + 1 opens the root part p left.  Panics as `page_circuit_witgen` does, but on `first >= D` (unless both
    /// are 0) where that refuses more updates than the trace has paths.
    pub fn page_circuit_witgen_part(&self, code: &HipBuffer<BabyBearElem>, proof: &HipBuffer<u32>, words: usize, nodes_before: &HipBuffer<BabyBearElem>,
                                    nodes_after: &HipBuffer<BabyBearElem>, first: usize, data: &HipBuffer<BabyBearElem>, steps: usize,
                                    noise_key: Option<&[u32; 8]>) -> [u32; 16] {
        let po2 = steps.trailing_zeros() as usize;
        let mut roots = [0u32; 16];
        ffi(|| unsafe { sys::zkh_page_circuit_witgen_part(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, code.raw, proof.raw, words, nodes_before.raw,
                                                          nodes_after.raw, first, data.raw, roots.as_mut_ptr(), noise_key.map_or(std::ptr::null(), |k| k.as_ptr())) });
        roots
    }

    /// The code group of P2-PAGE-ordered, P2-PAGE plus the constraint that the addresses strictly increase (`zkh_page_ordered_code`):
    /// P2-PAGE's 39 columns, then gsel, gpow, gend.  `self` holds the P2-PAGE-ordered description; `code` has 42 columns.  Panics as
    /// `page_circuit_code` does, and on an image of more than 2^29 words (h > 26: the gap between two addresses has 29 bits).
    pub fn page_ordered_code(&self, image_words: usize, code: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_page_ordered_code(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, image_words, code.raw) });
    }

    /// The data group of P2-PAGE-ordered for the part at `first` of a page-out (`zkh_page_ordered_witgen`), and the `out` globals: the
    /// root before update `first`, the root after the part's last update, then lo and hi as the trace holds them (Montgomery words): the
    /// part's live addresses strictly increase from lo on, and hi is one more than the last of them.  The operands are
    /// `page_circuit_witgen_part`'s, `data` has 129 columns; `first = 0` with D <= N is the single-seal case.  Part p + 1 opens the
    /// root and starts at the hi part p left.  Panics as `page_circuit_witgen_part` does.
    pub fn page_ordered_witgen(&self, code: &HipBuffer<BabyBearElem>, proof: &HipBuffer<u32>, words: usize, nodes_before: &HipBuffer<BabyBearElem>,
                               nodes_after: &HipBuffer<BabyBearElem>, first: usize, data: &HipBuffer<BabyBearElem>, steps: usize,
                               noise_key: Option<&[u32; 8]>) -> [u32; 18] {
        let po2 = steps.trailing_zeros() as usize;
        let mut out = [0u32; 18];
        ffi(|| unsafe { sys::zkh_page_ordered_witgen(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, code.raw, proof.raw, words, nodes_before.raw,
                                                     nodes_after.raw, first, data.raw, out.as_mut_ptr(), noise_key.map_or(std::ptr::null(), |k| k.as_ptr())) });
        out
    }

    /// The code group of P2-TREE, a page-out sealed by its dirty nodes (`zkh_page_tree_code`): 41 columns, a function of the trace's
    /// size alone, so one control root serves every image size.  `self` holds the P2-TREE description with its ZKA1 arguments set.
    pub fn page_tree_code(&self, code: &HipBuffer<BabyBearElem>, steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_page_tree_code(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, code.raw) });
    }

    /// The parts `(first, count)` of a page-out with the addresses `addrs` (strictly increasing, below `image_words`) as P2-TREE traces
    /// (`zkh_page_tree_plan`, host only): whole pairs of leaves while a part's dirty nodes fit the trace's block slots.
    pub fn page_tree_plan(image_words: usize, addrs: &[u32], steps: usize) -> Vec<(usize, usize)> {
        let po2 = steps.trailing_zeros() as usize;
        let cap = addrs.len().max(1);
        let (mut parts, mut n) = (vec![0usize; 2 * cap], 0usize);
        ffi(|| unsafe { sys::zkh_page_tree_plan(po2, sys::ZK_CYCLES, image_words, addrs.as_ptr(), addrs.len(), parts.as_mut_ptr(), cap, &mut n) });
        (0..n).map(|p| (parts[2 * p], parts[2 * p + 1])).collect()
    }

    /// `page_tree_plan` over a table that lies on the device (`zkh_page_tree_plan_device`): the words of `table` from `table_at` on are
    /// `rows` rows of a ZKU1 table (for a proof `table_at = 5 + h`).  Returns the parts and the dirty nodes of each; no word per row
    /// comes back to the host, so this host needs no copy of the table.  Panics on the refusals include/zkhal.h lists.
    pub fn page_tree_plan_device(&self, image_words: usize, table: &HipBuffer<u32>, table_at: usize, rows: usize, steps: usize) -> (Vec<(usize, usize)>, Vec<u32>) {
        let po2 = steps.trailing_zeros() as usize;
        let cap = rows.max(1);
        let (mut parts, mut nodes, mut n) = (vec![0usize; 2 * cap], vec![0u32; cap], 0usize);
        ffi(|| unsafe { sys::zkh_page_tree_plan_device(self.hal.ctx.0, po2, sys::ZK_CYCLES, image_words, table.raw, table_at, rows, parts.as_mut_ptr(), cap, &mut n,
                                                       nodes.as_mut_ptr()) });
        nodes.truncate(n);
        ((0..n).map(|p| (parts[2 * p], parts[2 * p + 1])).collect(), nodes)
    }

    /// The data group of P2-TREE for the part `[first, first + count)` of a page-out (`zkh_page_tree_witgen`), and the `out` globals:
    /// the root before the part, the root after it, then lo and hi (Montgomery words) bounding the heap ids of its pair blocks.  The
    /// other operands are `page_ordered_witgen`'s, `data` has 106 columns; the accum group comes from `zkh_accumulate`.  Part p + 1
    /// opens the root and starts at the hi part p left; part 0 starts at 2^(h-1).  Panics on the refusals include/zkhal.h lists.
    pub fn page_tree_witgen(&self, code: &HipBuffer<BabyBearElem>, proof: &HipBuffer<u32>, words: usize, nodes_before: &HipBuffer<BabyBearElem>,
                            nodes_after: &HipBuffer<BabyBearElem>, first: usize, count: usize, data: &HipBuffer<BabyBearElem>, steps: usize,
                            noise_key: Option<&[u32; 8]>) -> [u32; 18] {
        let po2 = steps.trailing_zeros() as usize;
        let mut out = [0u32; 18];
        ffi(|| unsafe { sys::zkh_page_tree_witgen(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, code.raw, proof.raw, words, nodes_before.raw,
                                                  nodes_after.raw, first, count, data.raw, out.as_mut_ptr(), noise_key.map_or(std::ptr::null(), |k| k.as_ptr())) });
        out
    }

    /// `page_tree_witgen` from (proof, dirty) alone (`zkh_page_tree_witgen_nodes`): `dirty`, the table `image_proof_nodes` left, stands
    /// in place of the two trees, for a rank that holds neither; the same cells and the same 18 words, for P2-TREE and P2-TREE-tied.
    /// Panics as `page_tree_witgen` does, on a table whose header does not fit its buffer or the proof, and on a table of another proof
    /// ("node N of layer K is not in the dirty nodes").
    pub fn page_tree_witgen_nodes(&self, code: &HipBuffer<BabyBearElem>, proof: &HipBuffer<u32>, words: usize, dirty: &HipBuffer<u32>, first: usize, count: usize,
                                  data: &HipBuffer<BabyBearElem>, steps: usize, noise_key: Option<&[u32; 8]>) -> [u32; 18] {
        let po2 = steps.trailing_zeros() as usize;
        let mut out = [0u32; 18];
        ffi(|| unsafe { sys::zkh_page_tree_witgen_nodes(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, code.raw, proof.raw, words, dirty.raw, first, count,
                                                        data.raw, out.as_mut_ptr(), noise_key.map_or(std::ptr::null(), |k| k.as_ptr())) });
        out
    }

    /// Check the raw traces against the circuit's own constraints on every row of `rows` (`zkh_check_rows`): which constraint a
    /// witness breaks, and where, before a seal is spent on it.  `out` and `mix` are the global words.  `row < 0`: no row of the window
    /// fails; otherwise the lowest failing row, its lowest failing `and_eqz` step (an index into the ZKC1 step list), how many rows of
    /// the window fail and the canonical value that step wants zero.  A failing row is an answer; it panics only on bad shapes, a bad
    /// window, or a step list whose live values exceed the step interpreter's LDS.
    pub fn check_rows(&self, accum: &HipBuffer<BabyBearElem>, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, out: &[u32], mix: &[u32],
                      steps: usize, rows: std::ops::Range<usize>, per_row: Option<&HipBuffer<u32>>) -> sys::ZkhCheckRowsResult {
        let po2 = steps.trailing_zeros() as usize;
        let g: [*const ZkhBuf; 3] = [accum.raw as *const ZkhBuf, ctrl.raw as *const ZkhBuf, data.raw as *const ZkhBuf];
        let mut res = sys::ZkhCheckRowsResult { row: -1, step: u32::MAX, failing_rows: 0, value: [0; 4] };
        ffi(|| unsafe { sys::zkh_check_rows(self.hal.ctx.0, self.circuit, po2, g.as_ptr(), 3, out.as_ptr(), mix.as_ptr(), rows.start, rows.end,
                                            per_row.map_or(std::ptr::null_mut(), |b| b.raw), &mut res) });
        res
    }

    /// Check the bus of the circuit's arguments key by key on the raw traces (`zkh_check_bus`): which key does not balance, when
    /// `accumulate` would only say that the bus does not.  No mix and no accum are involved.  `term < 0`: every key balances; otherwise
    /// the representative (lowest blob term index, then row) of the unbalanced key whose representative is lowest, the key, its net in
    /// Fp and how many of the distinct keys do not balance.  `per_term` (one record per term of the blob) receives what every term
    /// holds of that key: entries, first and last row, weight.  An unbalanced bus is an answer; it panics only on bad shapes, a circuit
    /// without arguments, or more keys than its table holds.
    pub fn check_bus(&self, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, steps: usize,
                     per_term: Option<&mut [sys::ZkhBusTerm]>) -> sys::ZkhCheckBusResult {
        let po2 = steps.trailing_zeros() as usize;
        let mut res = sys::ZkhCheckBusResult { row: -1, term: -1, tag: 0, key: [0; 4], net: 0, unbalanced_keys: 0, distinct_keys: 0, slots: 0 };
        let (terms, n_terms) = per_term.map_or((std::ptr::null_mut(), 0), |t| (t.as_mut_ptr(), t.len()));
        ffi(|| unsafe { sys::zkh_check_bus(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, ctrl.raw, data.raw, terms, n_terms, &mut res) });
        res
    }

    /// `(open tag, out offsets of alpha, beta, the total)` of arguments that are an OPEN bus (ZKA1 version 8; `zkh_circuit_open_bus`):
    /// a bus across seals, whose challenges and total are words of `out`.  `None`: the bus closes on zero inside the seal.
    pub fn open_bus(&self) -> Option<[u32; 4]> {
        let mut wh = [0u32; 4];
        if unsafe { sys::zkh_circuit_open_bus(self.circuit, wh.as_mut_ptr()) } != 0 { Some(wh) } else { None }
    }

    /// `accumulate` for an OPEN bus (`zkh_accumulate_open`): `challenge` = alpha ‖ beta where the mix globals were; returns the bus
    /// total, which the seal states in `out` behind the challenge.  It panics on a vanishing denominator and on a closed blob.
    pub fn accumulate_open(&self, ctrl: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, challenge: &[u32; 8], accum: &HipBuffer<BabyBearElem>,
                           steps: usize) -> [u32; 4] {
        let po2 = steps.trailing_zeros() as usize;
        let mut total = [0u32; 4];
        ffi(|| unsafe { sys::zkh_accumulate_open(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, std::ptr::null(), ctrl.raw, data.raw, challenge.as_ptr(), accum.raw,
                                                 total.as_mut_ptr()) });
        total
    }

    /// The root of the data group a seal of this circuit commits to, read out of the seal (`zkh_seal_data_root`; host only).
    pub fn seal_data_root(&self, seal: &[u32]) -> [u32; 8] {
        let mut root = [0u32; 8];
        ffi(|| unsafe { sys::zkh_seal_data_root(self.circuit, seal.as_ptr(), seal.len(), root.as_mut_ptr()) });
        root
    }

    /// The data columns that the four derives write on the active rows, ascending (`zkh_circuit_derived_data_columns`).
    pub fn derived_data_columns(&self) -> Vec<u32> {
        let mut n = 0usize;
        let mut cols = vec![0u32; 1 << 16];
        ffi(|| unsafe { sys::zkh_circuit_derived_data_columns(self.circuit, cols.as_mut_ptr(), cols.len(), &mut n) });
        cols.truncate(n);
        cols
    }

    /// Upload a caller's data trace from pinned memory without what the library derives (`zkh_upload_data_trace`): the other columns
    /// whole, the derived ones on their blinding rows only; enqueued on the stream, no host sync.
    pub fn upload_data_trace(&self, data: &HipBuffer<BabyBearElem>, pinned: &[u32], steps: usize) {
        let po2 = steps.trailing_zeros() as usize;
        ffi(|| unsafe { sys::zkh_upload_data_trace(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, data.raw, pinned.as_ptr(), 1) });
    }
}

impl Drop for HipCircuitHal {
    fn drop(&mut self) {
        unsafe { sys::zkh_circuit_destroy(self.circuit) }
    }
}

impl CircuitHal<HipHal> for HipCircuitHal {
    fn eval_check(&self, check: &HipBuffer<BabyBearElem>, groups: &[&HipBuffer<BabyBearElem>], globals: &[&HipBuffer<BabyBearElem>], poly_mix: BabyBearExtElem, po2: usize, steps: usize) {
        let g: Vec<*const ZkhBuf> = groups.iter().map(|b| b.raw as *const ZkhBuf).collect();
        let gl: Vec<*const ZkhBuf> = globals.iter().map(|b| b.raw as *const ZkhBuf).collect();
        debug_assert_eq!(check.size(), 4 * INV_RATE * steps); // CHECK_SIZE planes of 4n words: 4 x 4n
        ffi(|| unsafe { sys::zkh_eval_check(self.hal.ctx.0, self.circuit, check.raw, g.as_ptr(), g.len(), gl.as_ptr(), gl.len(), HipHal::ext_words(&poly_mix), po2, steps, 0) });
    }

    /// `CircuitHal::accumulate(ctrl, io, data, mix, accum, steps)`: for a circuit with arguments attached (`set_arguments`) the
    /// library's built-in accumulate fills `accum` from the raw code (ctrl) and data traces and the mix globals, blinding rows from
    /// fresh OS randomness; it panics on a refused witness (a vanishing denominator, a bus that does not balance) like every failed
    /// HAL op.  A circuit without arguments has no accumulate here: its host supplies one (`zkh_session_set_accumulate`).
    fn accumulate(&self, ctrl: &HipBuffer<BabyBearElem>, _io: &HipBuffer<BabyBearElem>, data: &HipBuffer<BabyBearElem>, mix: &HipBuffer<BabyBearElem>,
                  accum: &HipBuffer<BabyBearElem>, steps: usize) {
        assert!(self.has_arguments(), "accumulate: this circuit carries no arguments (HipCircuitHal::set_arguments)");
        let po2 = steps.trailing_zeros() as usize;
        let mix_words = mix.read_words(0, mix.size());
        ffi(|| unsafe { sys::zkh_accumulate(self.hal.ctx.0, self.circuit, po2, sys::ZK_CYCLES, std::ptr::null(), ctrl.raw, data.raw, mix_words.as_ptr(), accum.raw) });
    }
}

/// THE TIE: the fingerprint of the `rows` table rows at word `table_at` of `table`, where `zkh_page_out_proof` left them,
/// under `challenge` = alpha ‖ beta (`zkh_table_fingerprint`): what the open total of the tied segment must be.
pub fn table_fingerprint(hal: &HipHal, table: &HipBuffer<BabyBearElem>, table_at: usize, rows: usize, challenge: &[u32; 8]) -> [u32; 4] {
    let mut total = [0u32; 4];
    ffi(|| unsafe { sys::zkh_table_fingerprint(hal.ctx.0, table.raw, table_at, rows, challenge.as_ptr(), total.as_mut_ptr()) });
    total
}

/// The root a seal of `data` will carry for its data group, before the seal is made (`zkh_data_root`).
pub fn data_root(prover: *mut sys::ZkhProver, po2: usize, data: &HipBuffer<BabyBearElem>) -> [u32; 8] {
    let mut root = [0u32; 8];
    ffi(|| unsafe { sys::zkh_data_root(prover, po2, data.raw, root.as_mut_ptr()) });
    root
}

/// A data group committed once and kept for the seal (`zkh_commit_data`): coefficients, 4n evaluations and Merkle nodes in buffers of its
/// own, none of them the trace.  It holds no pointer to the prover that made it, so it may outlive that prover; like a `HipBuffer` it
/// must be dropped before the context.
pub struct HeldCommitment { raw: *mut sys::ZkhCommitment }

impl HeldCommitment {
    pub fn commit(prover: *mut sys::ZkhProver, po2: usize, data: &HipBuffer<BabyBearElem>) -> Self {
        let mut raw: *mut sys::ZkhCommitment = std::ptr::null_mut();
        ffi(|| unsafe { sys::zkh_commit_data(prover, po2, data.raw, &mut raw) });
        HeldCommitment { raw }
    }
    /// the root `data_root` gives for the same trace
    pub fn root(&self) -> [u32; 8] {
        let mut root = [0u32; 8];
        ffi(|| unsafe { sys::zkh_commitment_root(self.raw, root.as_mut_ptr()) });
        root
    }
    /// device bytes of the three buffers held, as the context counts live bytes
    pub fn bytes(&self) -> usize {
        unsafe { sys::zkh_commitment_bytes(self.raw) }
    }
}

impl Drop for HeldCommitment {
    fn drop(&mut self) {
        unsafe { sys::zkh_commitment_release(self.raw) };
    }
}

/// `zkh_prove_begin` from a held commitment (`zkh_prove_begin_held`): nothing of the data group is computed again, and the seal is the one
/// `zkh_prove_begin` of the committed trace gives.  The job takes references of its own: `held` may be dropped before `zkh_prove_finish`
/// and may seed further jobs.  `code` = None shares the prover's resident code group.  -> (the job, the mix challenges).
pub fn prove_begin_held(prover: *mut sys::ZkhProver, po2: usize, code: Option<&HipBuffer<BabyBearElem>>, held: &HeldCommitment, out_global: &[u32],
                        mix_words: usize) -> (*mut sys::ZkhSealJob, Vec<u32>) {
    let mut job: *mut sys::ZkhSealJob = std::ptr::null_mut();
    let mut mix = vec![0u32; mix_words.max(1)];
    let code_raw = code.map_or(std::ptr::null(), |c| c.raw as *const sys::ZkhBuf);
    ffi(|| unsafe { sys::zkh_prove_begin_held(prover, po2, code_raw, held.raw, out_global.as_ptr(), &mut job, mix.as_mut_ptr()) });
    mix.truncate(mix_words);
    (job, mix)
}

/// alpha ‖ beta of a tied group from its data roots in order, the segment's first (`zkh_tie_challenge`; host only): prover and
/// verifier call the same function.
pub fn tie_challenge(roots: &[[u32; 8]]) -> [u32; 8] {
    let mut challenge = [0u32; 8];
    ffi(|| unsafe { sys::zkh_tie_challenge(roots.as_ptr() as *const u32, roots.len(), challenge.as_mut_ptr()) });
    challenge
}

/// `SegmentProver::prove` in the two halves upstream drives `Prover` in, for hosts that would rather hand the library whole
/// traces than go op by op: `zkh_prove_begin` (header, commit code + data, draw the accum mix) -> the circuit's own
/// `accumulate` -> `zkh_prove_finish` (commit accum, eval_check, DEEP, FRI, queries).  Traces come from pinned memory
/// (`zkh_host_alloc`) through `zkh_write_async`: enqueued on the stream, no host sync.
pub fn prove_segment_from_host_traces(hal: &HipHal, prover: *mut sys::ZkhProver, po2: usize, code: &[u32], data: &[u32], out_global: &[u32], mix_words: usize,
                                      accumulate: impl FnOnce(&[u32], &HipBuffer<BabyBearElem>) -> HipBuffer<BabyBearElem>) -> Vec<u32> {
    let dcode = hal.alloc::<BabyBearElem>("code", code.len(), false);
    let ddata = hal.alloc::<BabyBearElem>("data", data.len(), false);
    ffi(|| unsafe { sys::zkh_write_async(hal.ctx.0, dcode.raw, code.as_ptr(), 0, code.len()) });
    ffi(|| unsafe { sys::zkh_write_async(hal.ctx.0, ddata.raw, data.as_ptr(), 0, data.len()) });
    let mut job: *mut sys::ZkhSealJob = std::ptr::null_mut();
    let mut mix = vec![0u32; mix_words.max(1)];
    ffi(|| unsafe { sys::zkh_prove_begin(prover, po2, dcode.raw, ddata.raw, out_global.as_ptr(), &mut job, mix.as_mut_ptr()) });
    let accum = accumulate(&mix[..mix_words], &ddata);
    let (mut seal, mut words): (*mut u32, usize) = (std::ptr::null_mut(), 0);
    ffi(|| unsafe { sys::zkh_prove_finish(job, accum.raw, &mut seal, &mut words) });
    let out = unsafe { std::slice::from_raw_parts(seal, words) }.to_vec();
    unsafe { sys::zkh_free_seal(seal) };
    out
}

/// `ProverServer::prove_session` + lift / join to ONE succinct receipt (risc0-zkvm 3.0.3 host/server/prove/prover_impl.rs), as the
/// library's session executor: `zkh_session_create` (G devices x K lanes), `zkh_session_build_recursion` (the lift / lift2 / join /
/// join3 — and, with assumptions, union / resolve — programs of a block with these segment sizes, BUILT by the library: no `.zkr` files), `zkh_session_prove(join_tree = 2)`
/// (seals and fold as one pipeline), and the root receipt's seal back.  `desc` = the segment circuit (`zkh_shipped_circuit_desc`
/// or the imported upstream tables), `segments` = (po2, seed) per segment, largest sizes first.
///
/// `chained` = Some((initial state, journal)) for a SYN-S circuit: the executor's pass gives every segment its pre-state and exit code, and the
/// LAST seal binds Output{SHA-256(journal), assumptions} — `journal` = the bytes the guest commits, for zeth the 32-byte block hash
/// (/root/reference/guests/stateless-client/src/lib.rs:33), which `cli.rs:103-107` then compares with `block.hash_slow()`.
pub fn prove_session_succinct(devices: &[i32], lanes_per_device: usize, desc: &[u32], segments: &[(u32, u64)],
                              assumptions: Option<(&[u32], &[AssumptionReceipt])>, chained: Option<(u32, &[u8])>) -> Vec<u32> {
    let mut session: *mut sys::ZkhSession = std::ptr::null_mut();
    ffi(|| unsafe { sys::zkh_session_create(devices.as_ptr(), devices.len(), lanes_per_device, desc.as_ptr(), desc.len(), std::ptr::null(), 0, &mut session) });
    if let Some((initial_state, journal)) = chained {
        ffi(|| unsafe { sys::zkh_session_set_chained(session, 1, initial_state) });
        ffi(|| unsafe { sys::zkh_session_set_journal(session, journal.as_ptr(), journal.len()) });
    }
    // `ProverServer::{union, resolve}`: the session's assumption receipts (keccak batches proven by `prove_keccak`) are handed over
    // BEFORE the programs are built; the executor lifts them, unites them pairwise and resolves the session's root against the union
    if let Some((adesc, receipts)) = assumptions {
        let seals: Vec<*const u32> = receipts.iter().map(|r| r.seal.as_ptr()).collect();
        let words: Vec<usize> = receipts.iter().map(|r| r.seal.len()).collect();
        let po2s: Vec<u32> = receipts.iter().map(|r| r.po2).collect();
        let roots: Vec<u32> = receipts.iter().flat_map(|r| r.control_root.iter().copied()).collect();
        ffi(|| unsafe { sys::zkh_session_set_assumptions(session, adesc.as_ptr(), adesc.len(), seals.as_ptr(), words.as_ptr(), po2s.as_ptr(), roots.as_ptr(), receipts.len()) });
    }
    let mut sizes: Vec<u32> = segments.iter().map(|s| s.0).collect();
    sizes.sort_unstable_by(|a, b| b.cmp(a));
    sizes.dedup();
    ffi(|| unsafe { sys::zkh_session_build_recursion(session, sizes.as_ptr(), sizes.len(), 1) });
    let segs: Vec<sys::ZkhSegment> = segments.iter().map(|&(po2, seed)| sys::ZkhSegment { po2, seed, ..unsafe { std::mem::zeroed() } }).collect();
    let mut info: sys::ZkhProveInfo = unsafe { std::mem::zeroed() };
    ffi(|| unsafe { sys::zkh_session_prove(session, segs.as_ptr(), segs.len(), 2, 0, std::ptr::null() /* a fresh OS key per fold proof */, &mut info) });
    ffi(|| unsafe { sys::zkh_session_verify(session, segs.as_ptr(), &info, 0) });
    let root = unsafe { std::slice::from_raw_parts(info.root_seal, info.root_seal_words) }.to_vec();
    unsafe { sys::zkh_prove_info_free(&mut info); sys::zkh_session_destroy(session) };
    root
}

/// One assumption receipt of a session: a seal of another circuit (KECCAK-F), its size, that circuit's control root at the size.
pub struct AssumptionReceipt { pub seal: Vec<u32>, pub po2: u32, pub control_root: [u32; 8] }

/// `verify_succinct` for a RESOLVED receipt: the claim is recomputed from the segment leaves AND the assumption receipts' claim digests
/// (the union tree sorts every pair; `leaves` empty: the receipt is the union-tree root alone).
pub fn verify_succinct_resolved(root_seal: &[u32], allowed_roots: &[[u32; 8]], root_program: usize, leaves: &[([u32; 8], u32, u32)], ranks: usize,
                                assumption_claims: &[[u32; 8]]) -> Result<(), String> {
    let flat_roots: Vec<u32> = allowed_roots.iter().flatten().copied().collect();
    let mut flat_leaves: Vec<u32> = Vec::with_capacity(10 * leaves.len());
    for (core, pre, post) in leaves { flat_leaves.extend_from_slice(core); flat_leaves.push(*pre); flat_leaves.push(*post); }
    let flat_claims: Vec<u32> = assumption_claims.iter().flatten().copied().collect();
    sys::ffi_wrap(|| unsafe {
        sys::zkh_succinct_verify_resolved(root_seal.as_ptr(), root_seal.len(), flat_roots.as_ptr(), allowed_roots.len(), root_program,
                                          flat_leaves.as_ptr(), leaves.len(), ranks, flat_claims.as_ptr(), assumption_claims.len())
    })
}

/// `SuccinctReceipt::verify_integrity` on the verifier's host (no GPU): one RECURSION seal under an allowed program's control
/// root, the allowed-programs root it carries, and its claim = the root of the leaves' claim tree (`leaves`: claim digest, pre, post).
pub fn verify_succinct(root_seal: &[u32], allowed_roots: &[[u32; 8]], root_program: usize, leaves: &[([u32; 8], u32, u32)], ranks: usize) -> Result<(), String> {
    let flat_roots: Vec<u32> = allowed_roots.iter().flatten().copied().collect();
    let mut flat_leaves: Vec<u32> = Vec::with_capacity(10 * leaves.len());
    for (core, pre, post) in leaves { flat_leaves.extend_from_slice(core); flat_leaves.push(*pre); flat_leaves.push(*post); }
    sys::ffi_wrap(|| unsafe {
        sys::zkh_succinct_verify(root_seal.as_ptr(), root_seal.len(), flat_roots.as_ptr(), allowed_roots.len(), root_program,
                                 flat_leaves.as_ptr(), leaves.len(), ranks)
    })
}

//! REPLACES the body of `MockProver::verify` in halo2_proofs 0.2.0 `src/dev.rs`: `MockProver::run` (synthesis into `fixed`, `advice`,
//! `instance`, `selectors`, `permutation`) stays upstream's; what it collected is checked on the device.  The gate polynomials of
//! all gates go down as `zk_expr_op` programs in ONE call, each lookup's expressions through the same evaluator and the
//! membership test, the copy constraints through the uploaded `Assembly` mapping; a status array becomes an ordered failure list.
//! NOT COMPILED here.  The Python mirror contangle-zkcp_amd/halo2.py (`MockProver`) is the tested statement of the same calls, and
//! DESIGN.md section 5 "MockProver" states the semantics and where they knowingly differ from upstream (no `CellNotAssigned`: an
//! unassigned cell is a stored 0; one `ConstraintPoisoned` per constraint; lookup failures ordered by (lookup, row)).
use zkcp_amd_sys as zk;

/// what `verify` needs after synthesis, already flattened by the caller: the columns advice ++ fixed ++ instance as resident
/// buffers of n Montgomery elements, the first Poison row of each, every gate polynomial as a stack program
pub struct DeviceCircuit<'a> {
    pub field: i32,
    pub k: u32,
    pub columns: &'a [zk::DeviceBuf],
    pub poison_from: &'a [u64],
    pub programs: &'a [zk::zk_expr_op],
    pub offsets: &'a [u32],
    pub consts: &'a [u64],
}

/// (index into the status array = program * n + row, byte: 1 = ConstraintNotSatisfied, 2 = ConstraintPoisoned), ascending
fn failures(status: &zk::DeviceBuf, len: usize, cap: usize, stream: *mut core::ffi::c_void) -> (Vec<(u64, u8)>, u64) {
    let (mut pos, mut kinds, mut total) = (vec![0u64; cap], vec![0u8; cap], 0u64);
    zk::check(unsafe { zk::zk_halo2_mock_failures_device(status.ptr() as _, len as u64, cap as u64, pos.as_mut_ptr(), kinds.as_mut_ptr(), &mut total,
                                                         stream) }, "zk_halo2_mock_failures_device").unwrap();
    let m = core::cmp::min(total as usize, cap);
    (pos[..m].iter().cloned().zip(kinds[..m].iter().cloned()).collect(), total)
}

/// every gate polynomial at every row: the (program, row, kind) triples `verify` turns into VerifyFailure values
pub fn gate_failures(c: &DeviceCircuit, cap: usize, stream: *mut core::ffi::c_void) -> (Vec<(u64, u8)>, u64) {
    let n = 1usize << c.k;
    let n_programs = c.offsets.len() - 1;
    let table: Vec<*const core::ffi::c_void> = c.columns.iter().map(|b| b.ptr() as *const core::ffi::c_void).collect();
    let status = zk::DeviceBuf::zeroed((n_programs * n + 7) / 8);
    zk::check(unsafe { zk::zk_halo2_mock_eval_device(c.field, c.k, c.programs.as_ptr(), c.offsets.as_ptr(), n_programs as u32, table.as_ptr(),
                                                     c.poison_from.as_ptr(), table.len() as u32, c.consts.as_ptr() as _, (c.consts.len() / 4) as u32,
                                                     core::ptr::null_mut(), status.ptr() as _, stream) }, "zk_halo2_mock_eval_device").unwrap();
    failures(&status, n_programs * n, cap, stream)
}

/// a lookup one expression wide: `inputs` / `table` are the evaluator's values, `*_status` its status bytes; rows that fail
pub fn lookup_failures(c: &DeviceCircuit, inputs: &zk::DeviceBuf, inputs_status: &zk::DeviceBuf, table: &zk::DeviceBuf, table_status: &zk::DeviceBuf,
                       usable_rows: usize, cap: usize, stream: *mut core::ffi::c_void) -> (Vec<(u64, u8)>, u64) {
    let status = zk::DeviceBuf::zeroed((usable_rows + 7) / 8);
    zk::check(unsafe { zk::zk_halo2_mock_lookup_device(c.field, c.k, inputs.ptr() as _, inputs_status.ptr() as _, table.ptr() as _, table_status.ptr() as _,
                                                       usable_rows as u64, status.ptr() as _, stream) }, "zk_halo2_mock_lookup_device").unwrap();
    failures(&status, usable_rows, cap, stream)
}

/// the copy constraints over the permutation's columns: (column * n + row) of every failing cell
pub fn permutation_failures(c: &DeviceCircuit, perm_columns: &[usize], mapping: &zk::DeviceBuf, cap: usize, stream: *mut core::ffi::c_void)
                            -> (Vec<(u64, u8)>, u64) {
    let n = 1usize << c.k;
    let table: Vec<*const core::ffi::c_void> = perm_columns.iter().map(|&i| c.columns[i].ptr() as *const core::ffi::c_void).collect();
    let poison: Vec<u64> = perm_columns.iter().map(|&i| c.poison_from[i]).collect();
    let status = zk::DeviceBuf::zeroed((table.len() * n + 7) / 8);
    zk::check(unsafe { zk::zk_halo2_mock_permutation_device(c.field, c.k, table.len() as u32, table.as_ptr(), poison.as_ptr(), mapping.ptr() as _,
                                                            status.ptr() as _, stream) }, "zk_halo2_mock_permutation_device").unwrap();
    failures(&status, table.len() * n, cap, stream)
}

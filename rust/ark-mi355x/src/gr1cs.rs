//! GR1CS on the device: every predicate of a constraint system, not only `"R1CS"`.
//!
//! `ConstraintSystem` keeps a `BTreeMap<Label, PredicateConstraintSystem>` (relations/src/gr1cs/constraint_system.rs:44-97)
//! and `to_matrices()` returns one list of matrices per label (:768-774).  `DeviceGr1cs::load` hands all of them, with each
//! predicate's polynomial (`get_all_predicate_types`, :178-183), to `ark355_gr1cs_load`; `which_is_unsatisfied` then answers
//! on the device what `ConstraintSystem::which_is_unsatisfied` (:661-687) answers on the host, in the same words
//! (`"<label> - <row>"`).
//!
//! Groth16 proves R1CS only.  `require_r1cs_only` is what `prove` and setup call before they take
//! `to_matrices()["R1CS"]`: a circuit with a constraint under any other predicate is refused instead of being proved as if
//! those constraints did not exist.
//!
//! UNCOMPILED in the repository's own build environment, like the rest of the crate.
use std::ffi::CString;

use ark_ff::PrimeField;
use ark_relations::gr1cs::{predicate::Predicate, ConstraintSynthesizer, ConstraintSystemRef, SynthesisError, R1CS_PREDICATE_LABEL};

use crate::error::Mi355xError;
use crate::{cache, ffi, marshal};

/// `Err` when a predicate other than `"R1CS"` carries a constraint (the error names it).
pub fn require_r1cs_only<F: PrimeField>(cs: &ConstraintSystemRef<F>) -> Result<(), Mi355xError> {
    for (label, n) in cs.get_all_predicates_num_constraints() {
        if label != R1CS_PREDICATE_LABEL && n > 0 {
            return Err(Mi355xError::InvalidArgument(format!(
                "predicate \"{label}\" carries {n} constraints: Groth16 proves R1CS only, and they would be dropped"
            )));
        }
    }
    Ok(())
}

/// A circuit that synthesises like `C` and then fails when a non-R1CS predicate carries a constraint: what setup hands to
/// the CPU generator, whose trait signature consumes the circuit.  The offending label is left in `refused`.
pub struct R1csOnly<'a, C> {
    pub circuit: C,
    pub refused: &'a core::cell::RefCell<Option<Mi355xError>>,
}

impl<'a, F: PrimeField, C: ConstraintSynthesizer<F>> ConstraintSynthesizer<F> for R1csOnly<'a, C> {
    fn generate_constraints(self, cs: ConstraintSystemRef<F>) -> Result<(), SynthesisError> {
        self.circuit.generate_constraints(cs.clone())?;
        if let Err(e) = require_r1cs_only(&cs) {
            *self.refused.borrow_mut() = Some(e);
            return Err(SynthesisError::PredicateNotFound); // the carrier only: the caller reports `refused`
        }
        Ok(())
    }
}

/// All predicates of one constraint system, resident on the device of this thread's context.
pub struct DeviceGr1cs {
    handle: *mut ffi::ark355_gr1cs,
    labels: Vec<String>,
    num_variables: usize,
}

impl DeviceGr1cs {
    /// `cs` must be finalized (`ConstraintSystemRef::finalize`), as for `to_matrices`.
    pub fn load<E: marshal::Mi355xCurve>(cs: &ConstraintSystemRef<E::ScalarField>) -> Result<Self, Mi355xError> {
        let mats = cs.to_matrices()?; // BTreeMap: sorted labels
        let types = cs.get_all_predicate_types();
        struct Flat<F: PrimeField> {
            label: CString,
            arity: u32,
            n: u64,
            term_coeff: Vec<F>,
            term_ptr: Vec<u32>,
            term_var: Vec<u32>,
            term_exp: Vec<u32>,
            csr: Vec<marshal::Csr<F>>,
            row_ptr: Vec<*const u64>,
            col: Vec<*const u32>,
            coeff: Vec<*const u8>,
        }
        let mut flat = Vec::with_capacity(mats.len());
        let mut labels = Vec::with_capacity(mats.len());
        for (label, ms) in &mats {
            let Predicate::Polynomial(p) = types.get(label).ok_or(SynthesisError::PredicateNotFound)?;
            let mut f = Flat {
                label: CString::new(label.as_str()).map_err(|_| Mi355xError::InvalidArgument("label contains a NUL".into()))?,
                arity: ms.len() as u32,
                n: ms.first().map_or(0, |m| m.len()) as u64,
                term_coeff: Vec::new(),
                term_ptr: vec![0],
                term_var: Vec::new(),
                term_exp: Vec::new(),
                csr: ms.iter().map(marshal::csr_from_matrix).collect(),
                row_ptr: Vec::new(),
                col: Vec::new(),
                coeff: Vec::new(),
            };
            for (c, term) in p.polynomial.terms.iter() {
                f.term_coeff.push(*c);
                for (var, exp) in term.iter() {
                    f.term_var.push(*var as u32);
                    f.term_exp.push(u32::try_from(*exp).map_err(|_| Mi355xError::InvalidArgument("exponent above u32".into()))?);
                }
                f.term_ptr.push(f.term_var.len() as u32);
            }
            f.row_ptr = f.csr.iter().map(|m| m.row_ptr.as_ptr()).collect();
            f.col = f.csr.iter().map(|m| m.col.as_ptr()).collect();
            f.coeff = f.csr.iter().map(|m| marshal::scalars_image(&m.coeff).as_ptr()).collect();
            labels.push(label.clone());
            flat.push(f);
        }
        let descs: Vec<ffi::ark355_predicate_desc> = flat
            .iter()
            .map(|f| ffi::ark355_predicate_desc {
                label: f.label.as_ptr(),
                arity: f.arity,
                n_constraints: f.n,
                n_terms: f.term_coeff.len() as u32,
                term_coeff: marshal::scalars_image(&f.term_coeff).as_ptr(),
                term_ptr: f.term_ptr.as_ptr(),
                term_var: f.term_var.as_ptr(),
                term_exp: f.term_exp.as_ptr(),
                row_ptr: f.row_ptr.as_ptr(),
                col: f.col.as_ptr(),
                coeff: f.coeff.as_ptr(),
            })
            .collect();
        let (ell, w) = (cs.num_instance_variables(), cs.num_witness_variables());
        let handle = cache::with_ctx(|ctx| {
            let mut h = core::ptr::null_mut();
            cache::check(ctx, unsafe {
                ffi::ark355_gr1cs_load(ctx, E::CURVE_ID, ell as u64, w as u64, descs.as_ptr(), descs.len() as u32, &mut h)
            })?;
            Ok(h)
        })?;
        Ok(Self { handle, labels, num_variables: ell + w })
    }

    /// constraint_system.rs:210-215
    pub fn num_constraints(&self) -> usize {
        unsafe { ffi::ark355_gr1cs_num_constraints(self.handle) as usize }
    }

    /// `ConstraintSystem::which_is_unsatisfied` (constraint_system.rs:661-687) for the full assignment
    /// `z = instance || witness`: `Some("<label> - <row>")` for the first unsatisfied constraint, labels in `BTreeMap` order.
    pub fn which_is_unsatisfied<F: PrimeField>(&self, z: &[F]) -> Result<Option<String>, Mi355xError> {
        if z.len() < self.num_variables {
            return Err(Mi355xError::Synthesis(SynthesisError::AssignmentMissing));
        }
        let (mut pred, mut row) = (-1i64, -1i64);
        cache::with_ctx(|ctx| {
            cache::check(ctx, unsafe {
                ffi::ark355_gr1cs_which_is_unsatisfied(ctx, self.handle, marshal::scalars_image(z).as_ptr(), z.len() as u64, &mut pred, &mut row)
            })
        })?;
        Ok(if pred < 0 { None } else { Some(format!("{} - {}", self.labels[pred as usize], row)) })
    }

    /// `is_satisfied` (constraint_system.rs:652-654)
    pub fn is_satisfied<F: PrimeField>(&self, z: &[F]) -> Result<bool, Mi355xError> {
        self.which_is_unsatisfied(z).map(|w| w.is_none())
    }
}

impl Drop for DeviceGr1cs {
    fn drop(&mut self) {
        unsafe { ffi::ark355_gr1cs_free(self.handle) }
    }
}

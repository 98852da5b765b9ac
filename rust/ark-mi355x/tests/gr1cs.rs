//! GR1CS through the shim, for a machine that has BOTH toolchains (Rust + ROCm with an MI355X): a circuit with a custom
//! gate -- a degree-5 S-box predicate `x0^5 - x1` next to ordinary R1CS rows.
//!  * `DeviceGr1cs::which_is_unsatisfied` answers what `ConstraintSystemRef::which_is_unsatisfied` answers on the host,
//!    in the same words (`"<label> - <row>"`), for a satisfied and an unsatisfied assignment;
//!  * `prove` and setup REFUSE the circuit instead of proving its R1CS rows alone.
use ark_bls12_381::{Bls12_381, Fr};
use ark_ff::Field;
use ark_mi355x::{DeviceGr1cs, Mi355xError, Mi355xGroth16};
use ark_relations::gr1cs::{
    predicate::PredicateConstraintSystem, ConstraintSynthesizer, ConstraintSystem, ConstraintSystemRef, LinearCombination,
    SynthesisError,
};
use ark_snark::{CircuitSpecificSetupSNARK, SNARK};
use ark_std::rand::{rngs::StdRng, SeedableRng};

const SBOX: &str = "s-box";

#[derive(Clone)]
struct SboxCircuit {
    x: Fr,
    /// what the circuit claims x^5 is
    y: Fr,
    sbox_rows: usize,
}

impl ConstraintSynthesizer<Fr> for SboxCircuit {
    fn generate_constraints(self, cs: ConstraintSystemRef<Fr>) -> Result<(), SynthesisError> {
        cs.register_predicate(SBOX, PredicateConstraintSystem::new_polynomial_predicate_cs(2, vec![(Fr::ONE, vec![(0, 5)]), (-Fr::ONE, vec![(1, 1)])]))?;
        let x = cs.new_witness_variable(|| Ok(self.x))?;
        let y = cs.new_input_variable(|| Ok(self.y))?;
        let x2 = cs.new_witness_variable(|| Ok(self.x.square()))?;
        cs.enforce_r1cs_constraint(|| LinearCombination::from(x), || LinearCombination::from(x), || LinearCombination::from(x2))?;
        for _ in 0..self.sbox_rows {
            cs.enforce_constraint_arity_2(SBOX, || LinearCombination::from(x), || LinearCombination::from(y))?;
        }
        Ok(())
    }
}

fn synthesized(c: SboxCircuit) -> (ConstraintSystemRef<Fr>, Vec<Fr>) {
    let cs = ConstraintSystem::<Fr>::new_ref();
    c.generate_constraints(cs.clone()).unwrap();
    cs.finalize();
    let mut z = cs.instance_assignment().unwrap();
    z.extend(cs.witness_assignment().unwrap());
    (cs, z)
}

#[test]
fn device_answers_like_the_host_for_every_predicate() {
    let x = Fr::from(3u64);
    for y in [x.pow([5u64]), Fr::from(7u64)] {
        let (cs, z) = synthesized(SboxCircuit { x, y, sbox_rows: 3 });
        let dev = DeviceGr1cs::load::<Bls12_381>(&cs).unwrap();
        assert_eq!(dev.num_constraints(), cs.num_constraints());
        assert_eq!(dev.which_is_unsatisfied(&z).unwrap(), cs.which_is_unsatisfied().unwrap());
    }
    let (cs, z) = synthesized(SboxCircuit { x, y: Fr::from(7u64), sbox_rows: 3 });
    assert_eq!(DeviceGr1cs::load::<Bls12_381>(&cs).unwrap().which_is_unsatisfied(&z).unwrap(), Some(format!("{SBOX} - 0")));
}

#[test]
fn groth16_refuses_a_circuit_with_a_custom_gate() {
    let mut rng = StdRng::seed_from_u64(7);
    let x = Fr::from(3u64);
    let gated = SboxCircuit { x, y: x.pow([5u64]), sbox_rows: 1 };
    let plain = SboxCircuit { sbox_rows: 0, ..gated.clone() };
    assert!(matches!(Mi355xGroth16::<Bls12_381>::setup(gated.clone(), &mut rng), Err(Mi355xError::InvalidArgument(m)) if m.contains(SBOX)));
    // a key for the R1CS rows alone must not yield a proof of the gated circuit either
    let (pk, _vk) = Mi355xGroth16::<Bls12_381>::setup(plain.clone(), &mut rng).unwrap();
    assert!(matches!(Mi355xGroth16::<Bls12_381>::prove(&pk, gated, &mut rng), Err(Mi355xError::InvalidArgument(m)) if m.contains(SBOX)));
    assert!(Mi355xGroth16::<Bls12_381>::prove(&pk, plain, &mut rng).is_ok());
}

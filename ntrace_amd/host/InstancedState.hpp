// InstancedState.hpp -- which of CudaInstancedBVH's derived products are current, and the one table that says which write voids which
// product.  A mutator of the class says what it writes -- wrote() only ever clears products -- and, after the library call
// succeeded, what it made; lost() is for a failed call that leaves a tree half-written.  Every predicate the class exposes is a pure
// function of the products.  A new derived product is one more Product, one more row of voidedBy() and one made() where it is computed:
// no other mutator changes.  No device code and no Buffer: tests/host/instanced_state_host_test.cpp exhausts this object on the host.
#pragma once

namespace FW {

class InstancedState {
public:
    enum class Write {     // what a call writes
        PoolTrees,         // the set of trees in the pool: addBLAS, buildBLASes
        PoolBoxes,         // the pool's boxes and Woop rows, the topology kept: refitBLASes
        PoolInnerBoxes,    // the pool's inner nodes only, node 0's box and the rows kept: optimizeBLASes
        Instances,         // the instances' transforms: setInstances, setInstancesDevice
        InstanceCount,     // ... with another count
        MotionKey,         // key 1 set or cleared: setMotionKey, setMotionKeyDevice, clearMotion
        World,             // setWorld, clearWorld
        TlasTopology,      // a build() starts
        TlasBoxes,         // the binary TLAS's boxes and the records: build, refit, refitMotion
        WidePool,          // the wide pool's nodes: widen, refitBLASesWide
        WideTlas,          // the wide TLAS and the wide records: widen, refitWide, refitMotionWide
        PoolKey1,          // the pool's key-1 buffers (second key's nodes, vertex rows, deforming flags): refitBLASesMotion, clearDeform
        Count
    };
    enum class Product {   // what can be current
        TlasTopology,      // a TLAS of the current instance count over the current BLASes exists: refit may run
        TlasBoxes,         // ... and its boxes and records are the current instances' and pool's: isBuilt()
        WideTopology,      // widen() has widened that topology: refitWide may run
        WidePool,
        WideTlas,          // the wide TLAS and the wide records
        FastFlags,         // ntr_instanced_validate's words over the binary buffers
        WideFastFlags,     // ntr_instanced_wide_validate's over the wide ones
        MotionRefit,       // the binary boxes are the swept ones, the records hold the moving flags
        WideMotionRefit,   // the same of the wide TLAS and records
        BlasTris,          // the device table of the meshes buildBLASes remembers
        PoolDeform,        // the pool's key-1 buffers and flags belong to the pool's current boxes: hasDeform()
        Count
    };
    explicit InstancedState(unsigned products = 0u) : m_products(products) {}

    // THE table: the writes that void a product.  A refit that starts keeps isBuilt() (only its failure is lost(TlasBoxes)), so TlasBoxes
    // is not voided by its own write; the wide TLAS is: widen() drops it before it writes.
    static constexpr unsigned voidedBy(Product p)
    {
        return p == Product::TlasTopology || p == Product::WideTopology ? bit(Write::PoolTrees) | bit(Write::InstanceCount) | bit(Write::TlasTopology)
             : p == Product::TlasBoxes ? voidedBy(Product::TlasTopology) | bit(Write::PoolBoxes) | bit(Write::Instances)
             : p == Product::WidePool ? bit(Write::PoolTrees) | bit(Write::PoolBoxes) | bit(Write::PoolInnerBoxes)
             : p == Product::WideTlas ? voidedBy(Product::WidePool) | bit(Write::TlasTopology) | bit(Write::TlasBoxes) | bit(Write::WideTlas)
             : p == Product::FastFlags ? voidedBy(Product::WidePool) | bit(Write::TlasTopology) | bit(Write::TlasBoxes) | bit(Write::World)
             : p == Product::WideFastFlags ? voidedBy(Product::FastFlags) | bit(Write::WidePool) | bit(Write::WideTlas)
             : p == Product::MotionRefit ? bit(Write::Instances) | bit(Write::InstanceCount) | bit(Write::MotionKey) | bit(Write::TlasTopology) | bit(Write::TlasBoxes)
                                          | bit(Write::PoolKey1)
             : p == Product::WideMotionRefit ? bit(Write::WideTlas)
             : p == Product::PoolDeform ? voidedBy(Product::WidePool)   // a plain refit or an optimize leaves the second key's nodes stale
             : /* BlasTris */ bit(Write::PoolTrees);
    }
    static constexpr bool voids(Write w, Product p) { return (voidedBy(p) & bit(w)) != 0u; }

    void wrote(Write w) { for (int p = 0; p < (int)Product::Count; p++) if (voids(w, (Product)p)) lost((Product)p); }
    void made(Product p) { m_products |= bit(p); }
    void lost(Product p) { m_products &= ~bit(p); }
    bool has(Product p) const { return (m_products & bit(p)) != 0u; }
    unsigned products(void) const { return m_products; }

    bool isBuilt(void) const { return has(Product::TlasBoxes); }
    bool isWidePoolCurrent(void) const { return has(Product::WidePool); }
    bool isWide(void) const { return isBuilt() && isWidePoolCurrent() && has(Product::WideTlas); }
    bool isFastFlagsStale(void) const { return !has(Product::FastFlags); }
    bool isWideFastFlagsStale(void) const { return !has(Product::WideFastFlags); }
    bool isMotionStale(void) const { return !has(Product::MotionRefit); }
    bool isPoolDeformCurrent(void) const { return has(Product::PoolDeform); }
    bool isMotionWideStale(void) const { return isMotionStale() || !has(Product::WideMotionRefit) || !has(Product::WideTlas); }
    bool mayRefit(void) const { return has(Product::TlasTopology); }
    bool mayRefitWide(void) const { return mayRefit() && has(Product::WideTopology); }

private:
    static constexpr unsigned bit(Write w) { return 1u << (int)w; }
    static constexpr unsigned bit(Product p) { return 1u << (int)p; }
    unsigned m_products;
};

}  // namespace FW
